"""Pictures with scaling matrices (TEST INFRASTRUCTURE), built at the CPU->GPU seam: everything from seeds, nothing is data.

A picture is taken from the stimulus modules that exist - tests/inter_stim.py (4 x 3 macroblocks: P, B with default and implicit
weights, explicit weights, the residual sweep with Intra16x16 / Intra4x4 / inter macroblocks at every QP), tests/t8x8_stim.py (4 x 3:
inter records with P264_MB_T8X8), tests/i8x8_stim.py (6 x 5: P and B pictures with Intra 8x8 macroblocks among inter ones) - or drawn
like theirs (I pictures of 6 x 5 with Intra16x16, Intra4x4 and Intra 8x8 macroblocks); `scaled` then gives it eight lists, optionally
new QPs, and brings it into range again with scaling_checker.make_conformant (the lists change what is in range).

The lists: JVT (the defaults of tables 7-3 / 7-4), random lists with weights 4 .. 64, lists that are 16 but for a few positions, and
a list set with a different weight at every scan position (a wrong scan -> raster mapping shows at once) - and the all-16 set, with
scaling_lists = 1: the flat decode through the scaled kernels.

`extreme_set()`: the rest of the byte - include/p264hip.h: "Any byte is legal (0 zeroes the coefficient)" - weights 1 .. 3, where the
rounding term of the right-shift branch dominates, 65 .. 255, where the 32-bit product is up to sixteen times a flat one, and 0.

`directed_set()`: the QPs on both sides of every branch (23 / 24, 35 / 36) for 4x4 blocks, the luma DC and 8x8 blocks, chroma DC of
both planes in intra and in inter macroblocks.  `random_set()`: drawn pictures over all QPs.  `assert_covered` says what the sets
must reach."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import i8x8_stim as IS
from tests import inter_stim as S
from tests import scaling_checker as SC
from tests import seam_fuzz
from tests import t8x8_stim as TS

Stim = collections.namedtuple("Stim", "name pic frames changed")      # changed: level blocks make_conformant had to shrink
THRESHOLD_QPS = (23, 24, 35, 36, 11, 12, 0, 51, 29, 30, 41, 42)
I_W, I_H = IS.MB_W, IS.MB_H


# ---- list sets -----------------------------------------------------------------------------------------------------------------
def jvt():
    return [list(x) for x in SC.DEFAULTS]


def random_lists(seed):
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.integers(4, 65, size=n)] for n in SC.SIZES]


def marked_lists(seed):
    """16 everywhere but for a few positions per list"""
    rng = np.random.default_rng(seed)
    out = []
    for n in SC.SIZES:
        lst = [16] * n
        for k in rng.choice(n, size=max(3, n // 5), replace=False):
            lst[int(k)] = int(rng.choice([4, 8, 12, 20, 24, 32, 40]))
        out.append(lst)
    return out


def ramp_lists():
    """a different weight at every scan position of every list"""
    return [[8 + 3 * n + k if size == 16 else 6 + n + (k * 37) % 61 for k in range(size)] for n, size in enumerate(SC.SIZES)]


def chosen_lists(seed, weights):
    """every position of every list drawn from `weights`"""
    rng = np.random.default_rng(seed)
    return [[int(v) for v in rng.choice(weights, size=n)] for n in SC.SIZES]


def flat_lists():
    return [list(x) for x in SC.FLAT]


# ---- one picture ---------------------------------------------------------------------------------------------------------------
def scaled(st, lists, name=None, qps=None):
    """the stimulus' picture with the eight lists (scaling_lists = 1) and, for qps = a sequence, macroblock m at QP qps[m % len]"""
    pic = st.pic
    if qps is not None:
        rec = pic.mb_records()
        for m in range(pic.n_mb):
            if int(rec["mb_type"][m]) != N.MB_IPCM:
                rec["qp"][m] = qps[m % len(qps)]
    SC.set_lists(pic, lists)
    _, changed = SC.make_conformant(pic) if pic.desc.n_coef_blocks else (0, 0)
    return Stim(name or "scaled " + st.name, pic, st.frames, changed)


def i_picture(rng, name, i8_share=0.4, deblock=True):
    """an I picture of 6 x 5: Intra16x16 and Intra4x4 macroblocks, a share of the Intra4x4 ones converted to Intra 8x8"""
    n = I_W * I_H
    force = {m: ("i16" if m % 3 == 0 else "i4") for m in range(n)}
    pic = seam_fuzz.make_picture(rng, I_W, I_H, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[0 if deblock else 1], force=force)
    SC.RC.make_conformant(pic)
    chosen = {m for m in range(n) if force[m] == "i4" and rng.random() < i8_share}
    IS.convert(pic, rng, chosen, IS.Plan(rng))
    return IS.Stim(name, pic, {}, 0, 0)


def _pick(stims, *names):
    by = {st.name: st for st in stims}
    return [by[n] for n in names]


def directed_set(seed=8590):
    rng = np.random.default_rng(seed)
    out = []
    q = THRESHOLD_QPS
    rot = lambda k: q[k:] + q[:k]
    # inter 4x4 blocks and chroma, Intra16x16 (luma DC) and Intra4x4 in P pictures: the residual sweep's pictures at the threshold QPs
    res = S.residual_set()
    for i, (st, lists) in enumerate(zip((res[0], res[6], res[12], res[18], res[24]), (jvt(), random_lists(1), ramp_lists(), marked_lists(2), random_lists(3)))):
        out.append(scaled(st, lists, "thresholds %s" % st.name, rot(i)))
    # 8x8 blocks of inter records: t8x8_stim's pictures, P / B / explicit weights, QPs on both sides of 36
    t8 = TS.directed_set()
    for i, (st, lists) in enumerate(zip(_pick(t8, "qp sweep 0", "quadrants", "P shapes", "B implicit road by road", "B default road by road", "mixed P weighted 0",
                                              "mixed B weighted 1", "around intra", "single levels 0"),
                                        (jvt(), random_lists(4), ramp_lists(), jvt(), random_lists(5), marked_lists(6), random_lists(7), ramp_lists(), ramp_lists()))):
        out.append(scaled(st, lists, "T8X8 %s" % st.name, None if st.name.startswith(("qp sweep", "single")) else rot(i)))
    # plain P, B and explicit-weight pictures
    for st, lists in zip(S.b_set()[:2] + S.weighted_set()[:1] + S.weighted_set()[2:3], (random_lists(8), jvt(), ramp_lists(), random_lists(9))):
        out.append(scaled(st, lists))
    # Intra 8x8 among inter macroblocks (6 x 5), and I pictures
    i8 = IS.inter_set()
    for i, (st, lists) in enumerate(zip(i8[:3] + i8[4:5], (jvt(), random_lists(10), ramp_lists(), random_lists(11)))):
        out.append(scaled(st, lists, "I8X8 %s" % st.name, rot(2 * i) if i < 2 else None))
    for i, lists in enumerate((jvt(), ramp_lists(), random_lists(12))):
        out.append(scaled(i_picture(rng, "I picture %d" % i, deblock=i != 1), lists, qps=rot(3 * i) if i < 2 else None))
    return out


def random_set(seed=8591):
    rng = np.random.default_rng(seed)
    out = []
    for i, st in enumerate(TS.random_set()[:4]):
        out.append(scaled(st, random_lists(100 + i) if i % 2 else marked_lists(100 + i)))
    for i, st in enumerate(IS.inter_set(seed=8600)[::2]):
        out.append(scaled(st, random_lists(110 + i)))
    out.append(scaled(i_picture(rng, "random I picture"), random_lists(120)))
    return out


LOW_QPS = (0, 5, 10, 14, 18, 22)
SMALL_WEIGHTS, LARGE_WEIGHTS, MIXED_WEIGHTS, ZERO_WEIGHTS = (1, 2, 3), (65, 96, 128, 160, 200, 254, 255), (1, 2, 3, 16, 65, 128, 255), (0, 16, 40)


def extreme_sources(seed):
    """six fresh pictures (`scaled` changes the one it is given): P residual sweeps with Intra16x16 / Intra4x4 / inter macroblocks, T8X8
    inter records, Intra 8x8 among inter macroblocks in a P and a B picture, an I picture"""
    res, i8 = S.residual_set(), IS.inter_set()
    return [res[0], res[12], TS.directed_set()[0], i8[0], i8[4], i_picture(np.random.default_rng(seed), "I picture")]


def extreme_set(seed=8597):
    """weights 1 .. 3 at the pictures' own QPs and at the threshold QPs; 65 .. 255, the whole byte mixed, and 0 beside 16 and 40 at QPs
    below 24.  (Large weights at high QPs are left out: 8.5.13's range leaves too few non-zero levels there - of the 968 level blocks of
    the six pictures make_conformant shrinks 382 at QPs (23, 24, 35, 36, 51, 30), 119 at LOW_QPS.)  Weight 0 is legal at the seam only:
    a stream's list cannot carry it."""
    out = []
    for k, (what, weights, qps) in enumerate((("weights 1..3", SMALL_WEIGHTS, None), ("weights 1..3 at the thresholds", SMALL_WEIGHTS, THRESHOLD_QPS),
                                              ("weights 65..255", LARGE_WEIGHTS, LOW_QPS), ("weights 1..255", MIXED_WEIGHTS, LOW_QPS),
                                              ("weights 0, 16, 40", ZERO_WEIGHTS, LOW_QPS))):
        for i, st in enumerate(extreme_sources(seed + k)):
            rot = None if qps is None else qps[i % len(qps):] + qps[:i % len(qps)]
            out.append(scaled(st, chosen_lists(seed + 10 * k + i, weights), "%s %s" % (what, st.name), rot))
    return out


def flat_twins(n=6):
    """pairs (picture with scaling_lists = 1 and all-16 lists, the same picture flat) of conformant pictures: P, B, explicit weights,
    T8X8, Intra 8x8, I"""
    rng = np.random.default_rng(8592)
    srcs = [lambda: S.residual_set()[3], lambda: _pick(TS.directed_set(), "quadrants")[0], lambda: S.b_set()[4], lambda: S.weighted_set()[0],
            lambda: IS.inter_set()[0], lambda: i_picture(np.random.default_rng(8593), "I twin")][:n]
    out = []
    for make in srcs:
        a, b = make(), make()
        out.append((scaled(a, flat_lists(), "all-16 " + a.name), Stim("flat " + b.name, b.pic, b.frames, 0)))
    return out


SETS = ("directed_set", "random_set", "extreme_set")


def survey(stims):
    c = SC.Census()
    for st in stims:
        _, bad = SC.census(st.pic, c)
        assert not bad, "%s: out of range %s" % (st.name, sorted(bad)[:3])
    return c


def assert_covered(which, stims):
    """AssertionError unless the pictures reach what the set is there for"""
    c = survey(stims)
    assert all(int(st.pic.desc.scaling_lists) for st in stims)
    changed, blocks = sum(st.changed for st in stims), sum(int(st.pic.desc.n_coef_blocks) for st in stims)
    assert changed * 5 <= blocks, "%s: %d of %d level blocks shrunk" % (which, changed, blocks)
    for n in range(8):
        assert c.lists[n] > 0, "list %d never met a non-zero level at a weight other than 16: %s" % (n, dict(c.lists))
    for plane in (1, 2):
        for kind in ("intra", "inter"):
            assert c.chroma_dc[(plane, kind)] > 0, "chroma DC of plane %d in %s macroblocks" % (plane, kind)
    kinds = set()
    for st in stims:
        d, rec = st.pic.desc, st.pic.mb_records()
        intra = rec["mb_type"] <= N.MB_IPCM
        kinds.add((int(d.slice_type), bool(d.explicit_wp), bool(d.weighted_bipred)))
        kinds.add("t8" if ((rec["intra_modes"] & N.MB_T8X8) != 0).any() else "no t8")
        kinds.add("i8" if ((rec["intra_modes"] & N.MB_I8X8) != 0).any() else "no i8")
        if int(d.slice_type) != N.SLICE_I and intra.any() and not intra.all():
            kinds.add("mixed")
    assert kinds >= {(N.SLICE_P, False, False), (N.SLICE_B, False, False), (N.SLICE_I, False, False), "t8", "i8", "mixed"}, kinds
    if which == "extreme_set":
        small, large, zero = SC.WEIGHT_CLASSES[1], SC.WEIGHT_CLASSES[3], SC.WEIGHT_CLASSES[0]
        for n in range(8):
            for cls in (small, large):
                assert c.classes[(n, cls)] > 0, "list %d never met a non-zero level at a weight of %s: %s" % (n, cls, sorted(c.classes.items()))
        assert any(c.classes[(n, zero)] for n in range(6)) and any(c.classes[(n, zero)] for n in (6, 7)), sorted(c.classes.items())
        for plane in (1, 2):
            for kind in ("intra", "inter"):
                assert c.dc_classes[((plane, kind), large)] > 0, "chroma DC of plane %d in %s macroblocks at a weight >= 65" % (plane, kind)
        assert c.dc_classes[("luma", large)] > 0 and c.dc_classes[("luma", small)] > 0, sorted(c.dc_classes.items())
        tables = [bytes(st.pic.desc.scaling4x4) + bytes(st.pic.desc.scaling8x8) for st in stims]
        assert {b for t in tables for b in t} >= {0, 1, 2, 3, 254, 255}
    if which != "directed_set":
        return
    assert kinds >= {(N.SLICE_B, False, True), (N.SLICE_P, True, False), (N.SLICE_B, True, False), "no t8", "no i8"}, kinds
    assert {(st.pic.mb_w, st.pic.mb_h) for st in stims} == {(S.MB_W, S.MB_H), (I_W, I_H)}
    have = {(rule, branch, qp) for rule, branch, qp in c.branches}
    for rule, lo in (("4x4", 24), ("luma dc", 36), ("8x8", 36)):
        assert (rule, "round", lo - 1) in have and (rule, "shift", lo) in have, "%s: qP %d / %d: %s" % (rule, lo - 1, lo, sorted(k for k in have if k[0] == rule))
