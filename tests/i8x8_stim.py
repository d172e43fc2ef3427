"""Pictures with Intra 8x8 macroblocks (TEST INFRASTRUCTURE), built at the CPU->GPU seam like tests/t8x8_stim.py's: everything from
seeds, nothing is data.

A picture is first drawn WITHOUT Intra 8x8 macroblocks (seam_fuzz.make_picture, or t8x8_stim.drawn_picture where inter
macroblocks are to carry N.MB_T8X8) and brought into range by residual_checker.make_conformant; then `convert` turns chosen I4x4
records into Intra 8x8 records (include/p264hip.h: P264_MB_I8X8): their 4x4 luma entries leave the coefficient stream, 8x8 blocks
of four entries each take their place, i4modes[4k .. 4k+3] get the block's mode, the descriptor gets N.T8X8_INTRA.  Levels: the
rule of residual_checker.make_conformant extended to 8x8 - a macroblock whose 8x8 blocks leave the range of 8.5.13 is redrawn with
halved levels until it is inside (`Stim.redrawn` counts them).

`avail` of a converted record is set DIRECTLY (as constrained intra prediction produces the sixteen combinations), inside what the
picture's borders allow, and the four modes are chosen for it: `Plan` walks the macroblocks and picks flags and modes that reach
a (mode, block, availability) case nobody has reached yet.

`dense_set()`: one I picture of 9 x 9 macroblocks (three bands of four rows: the hand-over between wavefronts carries Intra 8x8
neighbours) with I4x4, I16x16 and I_PCM macroblocks between the flagged ones.  `inter_set()`: P and B pictures of 6 x 5 macroblocks,
flagged macroblocks sparse and in clusters among inter macroblocks with and without N.MB_T8X8, explicit weights in one, QPs over
0 .. 51, loop filter on and off."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import i8x8_checker as I8
from tests import inter_stim as S
from tests import pcm_fuzz
from tests import residual_checker as RC
from tests import seam_fuzz
from tests import t8x8_checker as T8
from tests import t8x8_stim as TS

Stim = collections.namedtuple("Stim", "name pic frames drawn redrawn")
DENSE_W = DENSE_H = 9
MB_W, MB_H = 6, 5


def all_cases():
    """every legal (mode, block, (left, top, top-left, top-right)) of an Intra 8x8 block"""
    out = set()
    for a in range(16):
        L, T, TR, TL = bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT), bool(a & N.AVAIL_TOPLEFT)
        for k in range(4):
            av = I8.block_availability(k, L, T, TR, TL)
            out |= {(m, k, av) for m in I8.legal_modes(*av[:3])}
    return out


class Plan:
    """flags and modes for the macroblocks to convert, one after the other: whatever reaches most cases not reached so far"""

    def __init__(self, rng, every_avail=False):
        """every_avail: a combination of flags nobody has had yet goes first"""
        self.rng, self.seen, self.every_avail, self.avails = rng, set(), every_avail, set()

    def modes_for(self, avail):
        L, T, TR, TL = bool(avail & N.AVAIL_LEFT), bool(avail & N.AVAIL_TOP), bool(avail & N.AVAIL_TOPRIGHT), bool(avail & N.AVAIL_TOPLEFT)
        modes, new = [], 0
        for k in range(4):
            av = I8.block_availability(k, L, T, TR, TL)
            legal = I8.legal_modes(*av[:3])
            fresh = [m for m in legal if (m, k, av) not in self.seen]
            modes.append((fresh[0], av) if fresh else (int(self.rng.choice(legal)), av))
            new += bool(fresh)
        return modes, new

    def take(self, allowed):
        """allowed: the flags the picture's borders permit.  Returns (avail, [mode of block 0 .. 3])"""
        best = None
        for a in range(16):
            if a & ~allowed:
                continue
            modes, new = self.modes_for(a)
            new += 8 * (self.every_avail and a not in self.avails)
            if best is None or new > best[2]:
                best = (a, modes, new)
        a, modes, _ = best
        if best[2] == 0:                                   # nothing new anywhere: any of the sixteen
            a = int(self.rng.choice([x for x in range(16) if not x & ~allowed]))
            modes, _ = self.modes_for(a)
        for k, (m, av) in enumerate(modes):
            self.seen.add((m, k, av))
        self.avails.add(a)
        return a, [m for m, _ in modes]


def allowed_flags(pic, m):
    x, y, w = m % pic.mb_w, m // pic.mb_w, pic.mb_w
    return (N.AVAIL_LEFT if x > 0 else 0) | (N.AVAIL_TOP if y > 0 else 0) | (N.AVAIL_TOPRIGHT if y > 0 and x + 1 < w else 0) | (N.AVAIL_TOPLEFT if x > 0 and y > 0 else 0)


def convert(pic, rng, chosen, plan, coded=0.6, first=0):
    """the I4x4 macroblocks `chosen` become Intra 8x8 records.  Returns (macroblocks with levels, of them redrawn).  first: where the
    cycle of seven starts - 1: the first converted macroblock has all four blocks coded (a picture of one macroblock)."""
    rec = pic.mb_records()
    old = np.asarray(pic.coefs).reshape(-1, 16)
    out, drawn, redrawn, nth = [], 0, 0, first
    for m in range(pic.n_mb):
        r = rec[m]
        mask, at = int(r["coef_mask"]), int(r["coef_index"])
        mine = [old[at + i] for i in range(bin(mask & 0x3ffffff).count("1"))] if mask else []
        new_at = len(out)
        if m in chosen:
            assert int(r["mb_type"]) == N.MB_I4x4 and not mask & N.COEF_LUMA_DC, "macroblock %d: I4x4 expected" % m
            has_dc = 1 if mask & N.COEF_CHROMA_DC else 0
            mine = mine[:has_dc] + mine[has_dc + bin(mask & 0xffff).count("1"):]
            avail, modes = plan.take(allowed_flags(pic, m))
            qp = int(r["qp"])
            share = (0.0, 1.0)[nth % 7] if nth % 7 < 2 else coded      # (every seventh none of the four blocks, the next one all)
            nth += 1
            lv = {k: TS.draw_block(rng, qp) for k in range(4) if rng.random() < share}
            drawn += bool(lv)
            hit = False
            for _ in range(24):
                rng_ = RC.Range()
                for v in lv.values():
                    T8.block8x8(v, qp, rng_)
                if rng_.ok:
                    break
                lv, hit = {k: TS.halve(v) for k, v in lv.items()}, True
            assert rng_.ok
            redrawn += hit
            luma = [v[16 * j:16 * j + 16].astype(np.int16) for k in sorted(lv) for v in [lv[k]] for j in range(4)]
            mine = mine[:has_dc] + luma + mine[has_dc:]
            r["coef_mask"] = (mask & ~0xffff) | sum(0xF << (4 * k) for k in lv)
            r["cbp"] = (int(r["cbp"]) & 0x30) | sum(1 << k for k in lv)
            r["intra_modes"] = N.MB_I8X8                   # (chroma DC: legal under any flags)
            r["avail"] = avail
            pic.i4modes[m * 16:m * 16 + 16] = np.repeat(np.array(modes, np.uint8), 4)
        r["coef_index"] = new_at
        out += mine
    pic.desc.n_coef_blocks = len(out)
    pic.coefs = np.concatenate(out + [np.zeros(16, np.int16)]).astype(np.int16)
    pic.desc.transform_8x8 = int(pic.desc.transform_8x8) | N.T8X8_INTRA
    pic.seal()
    return drawn, redrawn


def dense_picture(rng, plan, name="dense I 9x9", deblock=True, mb_w=DENSE_W, mb_h=DENSE_H):
    w, h = mb_w, mb_h
    n = w * h
    plain = [m for m in range(n) if ((m % w) + 3 * (m // w)) % 4 == 0]        # the macroblocks that stay what they are
    kinds = {m: ("i4", "i16", "ipcm")[i % 3] for i, m in enumerate(plain)}
    force = {m: "i4" for m in range(n) if m not in kinds}
    force.update({m: k for m, k in kinds.items() if k != "ipcm"})
    pic = seam_fuzz.make_picture(rng, w, h, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[0 if deblock else 1], force=force)
    chosen = np.zeros(n, bool)
    chosen[[m for m, k in kinds.items() if k == "ipcm"]] = True
    pcm_fuzz.to_ipcm(rng, pic, 0, samples="noise", chosen=chosen)
    RC.make_conformant(pic)
    drawn, redrawn = convert(pic, rng, {m for m in range(n) if m not in kinds}, plan)
    return Stim(name, pic, {}, drawn, redrawn)


def dense_set(seed=8322):
    rng = np.random.default_rng(seed)
    return [dense_picture(rng, Plan(rng))]


# clusters and single macroblocks of a 6 x 5 picture (none on the border: all sixteen flag combinations are open to them)
CLUSTER = (7, 8, 9, 13, 14, 15, 20)
SPARSE = (7, 10, 16, 21, 27)


def inter_picture(rng, plan, name, flagged, t8_share, mb_w=MB_W, mb_h=MB_H, **kw):
    st = TS.drawn_picture(rng, name, mb_w, mb_h, share=t8_share, intra_share=0.1, force={m: "i4" for m in flagged}, **kw)
    pic = st.pic
    if not (pic.mb_records()["intra_modes"] & N.MB_T8X8).any():
        pic.desc.transform_8x8 = 0                         # (no inter record carries the flag: Intra 8x8 alone)
    rec = pic.mb_records()
    chosen = set(flagged) | {m for m in range(pic.n_mb) if int(rec["mb_type"][m]) == N.MB_I4x4 and rng.random() < 0.5}
    drawn, redrawn = convert(pic, rng, chosen, plan)
    return Stim(name, pic, st.frames, st.drawn + drawn, st.redrawn + redrawn)


def inter_set(seed=8323):
    rng = np.random.default_rng(seed)
    plan = Plan(rng, every_avail=True)
    return [inter_picture(rng, plan, "P cluster", CLUSTER, 0.5, slices=1, slice_idcs=[0]),
            inter_picture(rng, plan, "P sparse without T8X8", SPARSE, 0.0, slices=1, slice_idcs=[0]),
            inter_picture(rng, plan, "P cluster weighted", CLUSTER, 0.5, explicit_wp="legal", slices=2, slice_idcs=[0, 2]),
            inter_picture(rng, plan, "P sparse unfiltered", SPARSE, 0.6, slices=1, slice_idcs=[1]),
            inter_picture(rng, plan, "B cluster", CLUSTER, 0.5, b_picture=True, slices=1, slice_idcs=[0]),
            inter_picture(rng, plan, "B sparse", SPARSE, 0.7, b_picture=True, slices=2, slice_idcs=[0])]


SETS = ("dense_set", "inter_set")


def cases_of(stims):
    """the (mode, block, availability) cases the pictures' records hold"""
    out = set()
    for st in stims:
        rec = st.pic.mb_records()
        for m in np.flatnonzero((rec["intra_modes"] & N.MB_I8X8) != 0):
            a = int(rec["avail"][m])
            for k in range(4):
                av = I8.block_availability(k, bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT), bool(a & N.AVAIL_TOPLEFT))
                out.add((int(st.pic.i4modes[m * 16 + 4 * k]), k, av))
    return out


def assert_covered(which, stims):
    """AssertionError unless the pictures reach what the set is there for (the CPU test on the drawn sets, the GPU file on what it
    submitted)"""
    fl = lambda st: (st.pic.mb_records()["intra_modes"] & N.MB_I8X8) != 0
    drawn, redrawn = sum(st.drawn for st in stims), sum(st.redrawn for st in stims)
    assert drawn and redrawn * 10 <= drawn, "%s: %d of %d macroblocks redrawn with halved levels" % (which, redrawn, drawn)
    for st in stims:
        rec = st.pic.mb_records()
        assert int(st.pic.desc.transform_8x8) & N.T8X8_INTRA and fl(st).any(), st.name
        for m in np.flatnonzero(fl(st)):
            assert I8.luma8x8_of(st.pic, int(m), refuse=False)[1].ok, "%s macroblock %d out of range" % (st.name, m)
    nibbles = {int(v) & 0xffff for st in stims for v in st.pic.mb_records()["coef_mask"][fl(st)]}
    assert nibbles >= {0, 0xffff} and len(nibbles) >= 6, sorted(hex(x) for x in nibbles)
    if which == "dense_set":
        assert {(st.pic.mb_w, st.pic.mb_h) for st in stims} == {(DENSE_W, DENSE_H)}
        assert all(int(st.pic.desc.slice_type) == N.SLICE_I for st in stims)
        missing = all_cases() - cases_of(stims)
        assert not missing, sorted(missing)
        beside = set()
        for st in stims:
            rec, f, w, h = st.pic.mb_records(), fl(st), st.pic.mb_w, st.pic.mb_h
            for m in np.flatnonzero(f):
                x, y = m % w, m // w
                for side, ok, nb in (("left", x > 0, m - 1), ("right", x + 1 < w, m + 1), ("top", y > 0, m - w), ("bottom", y + 1 < h, m + w)):
                    if ok:
                        beside.add(("i8" if f[nb] else int(rec["mb_type"][nb]), side))
        for kind in ("i8", N.MB_I4x4, N.MB_I16x16, N.MB_IPCM):
            for side in ("left", "right", "top", "bottom"):
                assert (kind, side) in beside, (kind, side)
        return
    kinds, avails, qps, beside = set(), set(), set(), set()
    for st in stims:
        rec, f, d = st.pic.mb_records(), fl(st), st.pic.desc
        t8 = (rec["intra_modes"] & N.MB_T8X8) != 0
        kinds.add((int(d.slice_type), bool(d.explicit_wp), bool(d.deblock), bool(t8.any())))
        w, h = st.pic.mb_w, st.pic.mb_h
        for m in np.flatnonzero(f):
            avails.add(int(rec["avail"][m]))
            if int(rec["coef_mask"][m]) & 0xffff:
                qps.add((int(rec["qp"][m]) % 6, int(rec["qp"][m]) >= 36))
            x, y = m % w, m // w
            for ok, nb in ((x > 0, m - 1), (x + 1 < w, m + 1), (y > 0, m - w), (y + 1 < h, m + w)):
                if ok:
                    beside.add("i8" if f[nb] else "t8" if t8[nb] else "inter" if rec["mb_type"][nb] > N.MB_IPCM else "intra")
    assert {k[0] for k in kinds} == {N.SLICE_P, N.SLICE_B} and any(k[1] for k in kinds), kinds
    assert {k[2] for k in kinds} == {True, False} and {k[3] for k in kinds} == {True, False}, kinds
    assert avails == set(range(16)), sorted(set(range(16)) - avails)
    assert {hi for _, hi in qps} == {True, False} and {m for m, _ in qps} == set(range(6)), sorted(qps)
    assert beside >= {"i8", "t8", "inter"}, beside
