"""tests/batch_kinds.py on the CPU: every kind is what its name says (counted from its records); cover() leaves no reachable (kind,
instance tuple) cell out; tuple_of is the C++ plan (the g++ program of tests/test_launch_plan_cpu.py); the expectation used on the GPU
(cr_offset_checker.TwoChains over scaling_checker.SpecRecon) is, byte for byte, the oracle's picture for the seven kinds of
tests/test_gpu_batch_composition.py; and what the earlier mixed-batch tests reach is a subset of what the cover reaches."""
import collections
import itertools

import numpy as np
import pytest

from tests import batch_kinds as BK
from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import hip_harness as H
from tests import i8x8_stim as IS
from tests import inter_stim
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import seam_fuzz
from tests import stream_args
from tests import t8x8_stim as TS
from tests import wp_checker
from tests.test_launch_plan_cpu import CU, plan          # noqa: F401 (plan: the fixture that compiles launch_plan.h with g++)

LARGE_W, LARGE_H = BK.LARGE_W, BK.LARGE_H
EARLIER = (85, 26, 607)           # cells and tuples of the earlier files, cells of the cover - by flags_of, not by name


# ---- the kinds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(BK.W, BK.H), (LARGE_W, LARGE_H)])
def test_every_kind_is_what_its_name_says(geometry):
    pics = BK.pictures(1405, *geometry)
    assert list(pics) == BK.NAMES and len(pics) >= 30
    reach = collections.Counter()
    for kind in BK.KINDS:
        pic = pics[kind.name].pic
        c, f = BK.census(pic), BK.flags_of(pic)
        what = "%s at %s: %s %s" % (kind.name, geometry, dict(c), f)
        assert (pic.mb_w, pic.mb_h) == geometry and int(pic.desc.dst_slot) == BK.DST, what
        assert set(int(pic.desc.ref_slot[i]) for i in range(int(pic.desc.n_ref))) <= {1, 2}, what
        assert not BK.missing(kind, pic), what
        # the name's first letter is the slice type; the flags are what the census counted
        assert (f["i"], f["p"], f["b"]) == {"I": (True, False, False), "P": (False, True, False), "B": (False, True, True)}[kind.name[0]], what
        assert f["wp"] == ("wp" in kind.has) and f["t8"] == ("t8" in kind.has) and f["i8"] == ("i8" in kind.has), what
        assert f["dup"] == ("dup" in kind.has) and f["cr"] == ("cr" in kind.has) and f["sc"] == int("lists" in kind.has or "cr" in kind.has), what
        if "dup" in kind.has:
            assert c["dup"] >= 2, what                         # macroblocks at both indices of the frame that list 0 holds twice
            tells = BK.dup_tells(pics[kind.name])               # ... and samples that a filter comparing indices, not pictures, gets wrong
            assert tells >= BK.DUP_TELLS, "%s: %d samples tell" % (what, tells)
        if "ipcm" in kind.has:
            assert c["ipcm"] and c["ipcm"] < pic.n_mb, what
        if "cr" in kind.has:
            assert c["cr"] and BK.v_differs(pics[kind.name]), what          # (Cr's offset changes samples of the picture)
            CR.reach(pic, reach)
        # inside the ranges of 8.5 under both chroma offsets: a second call changes nothing
        before = pic.coefs.tobytes() + pic.mb_records().tobytes()
        if int(pic.desc.n_coef_blocks):
            CR.make_conformant(pic, SC.make_conformant)
        assert pic.coefs.tobytes() + pic.mb_records().tobytes() == before, what
    if geometry == (BK.W, BK.H):
        CR.assert_reached(reach)                                # (the set of Cr kinds: edges of every class and strength, both clips, I_PCM)
    else:
        assert sum(k[0] == "edge" for k in reach) >= 6, sorted(reach)     # (several classes and strengths of edge where Cr's QPc differs)


def test_the_seven_old_kinds_are_those_of_the_composition_test():
    assert BK.OLD == list(stream_args.KINDS)
    f = BK.kind_flags()
    sig = lambda fl: tuple(int(fl[x]) for x in BK.FLAGS)
    rng = np.random.default_rng(5)
    for name in BK.OLD:
        assert sig(f[name]) == sig(BK.flags_of(stream_args.draw(rng, 5, 4, name))), name


# ---- the cells ---------------------------------------------------------------------------------------------------------------------
def test_cover_reaches_every_cell_and_every_tuple():
    cover = BK.cover()
    assert len(set(cover)) == len(cover) and cover[:len(BK.NAMES)] == [(n,) for n in BK.NAMES] and cover[len(BK.NAMES)] == tuple(BK.NAMES)
    assert all(len(m) <= 4 for m in cover[len(BK.NAMES) + 1:])
    reached = set().union(*(BK.cells_of(m) for m in cover))
    within_four = set()
    for members in BK.subsets(4):
        within_four |= BK.cells_of(members)
    tuples = set(BK.every_tuple())
    old = set().union(*(BK.cells_of(m) for m in BK.subsets(len(BK.OLD), BK.OLD)))
    simple = set().union(*(BK.cells_of(m) for m in list(BK.subsets(2)) + [tuple(BK.NAMES)]))
    counts = "%d kinds: %d tuples (the seven old kinds: %d), %d cells within four (singles, pairs and the full set: %d), cover: %d subsets, %d cells, %d tuples" % (
        len(BK.NAMES), len(tuples), len({t for _, t in old}), len(within_four), len(simple), len(cover), len(reached), len({t for _, t in reached}))
    print(counts)
    assert within_four <= reached, "%s; missing %s" % (counts, sorted(within_four - reached)[:5])
    assert tuples == {t for _, t in reached}, "%s; missing %s" % (counts, sorted(tuples - {t for _, t in reached}))
    # the closure is what brute force finds where brute force is affordable: every subset of the first 14 kinds
    few = BK.NAMES[:14]
    brute = {BK.tuple_of(m) for m in BK.subsets(len(few), few)}
    assert brute <= tuples
    assert (len(BK.NAMES), len(tuples), len(within_four), len(cover)) == (36, 64, 715, 239), counts       # (the figures of DESIGN section 5)


def test_cover_is_deterministic():
    BK.cover.cache_clear()
    a = list(BK.cover())
    BK.cover.cache_clear()
    assert a == BK.cover()


def test_tuple_of_is_the_plan(plan):
    rng = np.random.default_rng(2000)
    batches = list(BK.cover()) + [tuple(str(x) for x in rng.choice(BK.NAMES, size=int(rng.integers(1, len(BK.NAMES) + 1)), replace=False)) for _ in range(2000)]
    f = BK.kind_flags()
    cases = []
    for members in batches:
        k = BK.union(f[m] for m in members)
        cases.append((BK.W, BK.H, len(members), CU, k, {}))
    for members, case, got in zip(batches, cases, plan(cases)):
        want = BK.plan_rules(case[4], len(members), None, BK.W * BK.H)
        assert {x: got[x] for x in want} == want, (members, got)
        assert tuple(got[x] for x in BK.TUPLE) == BK.tuple_of(members), (members, got)
        assert got["scaled_pictures"] == sum(f[m]["sc"] for m in members) and got["cr_pictures"] == sum(f[m]["cr"] for m in members)


# ---- the expectation ---------------------------------------------------------------------------------------------------------------
def test_the_spec_model_is_the_oracle_on_the_old_kinds(oracle):
    for name in BK.OLD:
        st = BK.pictures()[name]
        chk = wp_checker.WeightedChecker(oracle, BK.W, BK.H, BK.SLOTS)
        for slot, frame in st.frames.items():
            for dst, src in zip(chk.store[slot], frame):
                dst[:] = src
        d = H.first_difference(BK.expected(st), chk.reconstruct(st.pic), "%s: the spec model against the oracle" % name, st.pic)
        assert d is None, d


# ---- what the earlier files reach --------------------------------------------------------------------------------------------------
def _dense_i8(rng, i):
    """tests/test_gpu_i8x8.py: small_dense, without its expectation"""
    from tests import residual_checker as RC
    w, h = IS.MB_W, IS.MB_H
    pic = seam_fuzz.make_picture(rng, w, h, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[i % 2], force={m: "i4" for m in range(w * h) if m % 5})
    RC.make_conformant(pic)
    IS.convert(pic, rng, {m for m in range(w * h) if m % 5}, IS.Plan(rng))
    return pic


def _plain(rng, **kw):
    """tests/test_gpu_i8x8.py: plain_picture, without its expectation"""
    kw.setdefault("n_ref", 2)
    kw.setdefault("n_ref_l1", 2)
    return seam_fuzz.make_picture(rng, IS.MB_W, IS.MB_H, slots=3, dst_slot=0, level_style="small", qp_mode="random", mv_range=40, **kw)


_Pic = collections.namedtuple("_Pic", "pic")


def earlier_batches():
    """the batches (lists of pictures) of tests/test_gpu_batch_composition.py and of the mixed-batch tests of tests/test_gpu_t8x8.py,
    test_gpu_i8x8.py, test_gpu_scaling.py and test_gpu_cr_offset_batches.py: their stimulus lists, batched as hip_harness.run_batches
    does (batches_of); the pictures' descriptors are all that is read"""
    out = []

    def batches(pics, n=3):
        out.extend([st.pic for st, _ in b] for b in H.batches_of([(_Pic(p), None) for p in pics], n))
    # the composition test: alone, in pairs, all together (its large batch of random kinds selects what `all together` selects)
    rng = np.random.default_rng(1016)
    comp = [stream_args.draw(rng, 5, 4, kind) for kind in stream_args.KINDS]
    out.extend([comp[s] for s in members] for members in [(s,) for s in range(7)] + list(itertools.combinations(range(7), 2)) + [tuple(range(7))])
    # test_gpu_t8x8.py::test_mixed_batches_and_what_the_launch_reports
    d = {st.name: st.pic for st in TS.directed_set()}
    plain = [st.pic for st in inter_stim.window_set()[:2] + inter_stim.b_set()[:1] + inter_stim.weighted_set()[:1]]
    batches([d["P shapes"], plain[2], d["mixed P weighted 0"], plain[0], d["B implicit road by road"], plain[3], d["mixed B weighted 1"], plain[1], d["quadrants"]])
    batches(plain[:3])
    # test_gpu_i8x8.py::test_mixed_batches_and_what_the_launch_reports
    rng = np.random.default_rng(8326)
    i8 = {st.name: st.pic for st in IS.inter_set()}
    t8_only = TS.drawn_picture(rng, "P with T8X8 alone", IS.MB_W, IS.MB_H, share=0.7, intra_share=0.1, slices=1, slice_idcs=[0]).pic
    plain = [_plain(rng, b_picture=True), _plain(rng), _plain(rng, slices=2), _plain(rng, p_picture=False)]
    batches([_dense_i8(np.random.default_rng(8324), 0), i8["P cluster"], t8_only, plain[0]], 4)
    for b in ([t8_only, plain[0], plain[1]], plain[:3], [plain[3], plain[1], plain[2]]):
        batches(b)
    # test_gpu_scaling.py::test_a_mixed_batch_and_what_the_launch_reports
    d = {st.name: st.pic for st in SS.directed_set()}
    rng = np.random.default_rng(8595)
    flat_p = seam_fuzz.make_picture(rng, IS.MB_W, IS.MB_H, n_ref=2, slots=3, dst_slot=0, level_style="small", qp_mode="random", intra_share=0.1)
    i8 = [st.pic for st in IS.inter_set(seed=8596)]
    flat = [flat_p, i8[0], i8[1], i8[4]]
    mixed = [d["I8X8 P cluster"], flat[0], d["I8X8 B cluster"], flat[1], d["I8X8 P cluster weighted"], flat[2], d["scaled I picture 0"], flat[3]]
    batches(mixed, 8)
    batches(mixed[:6], 6)
    batches(flat, 4)
    # test_gpu_cr_offset_batches.py, all of it
    with_delta, without = [st.pic for st in CS.batch_set()], [st.pic for st in CS.flat_set()]
    mixed = [p for pair in zip(with_delta, without) for p in pair]
    for n in (1, 2, 3, 5):
        batches(mixed, n)
    batches(without, 4)
    batches(without[:-1] + [p for p in with_delta if int(p.desc.slice_type) == int(without[-1].desc.slice_type)][:1], 4)
    return out


def test_the_earlier_files_reach_a_subset_of_the_cover():
    """cells by what a picture contributes to BatchKinds (its flags_of) instead of by a kind's name: the earlier files' pictures are not
    drawn from the table"""
    sig = lambda fl: tuple(int(fl[x]) for x in BK.FLAGS)
    f = BK.kind_flags()
    new = set()
    for members in BK.cover():
        t = BK.tuple_of(members)
        new |= {(sig(f[m]), t) for m in members}
    earlier = set()
    for batch in earlier_batches():
        flags = [BK.flags_of(p) for p in batch]
        t = BK.tuple_of_flags(flags)
        earlier |= {(sig(fl), t) for fl in flags}
    counts = "the earlier files reach %d cells of %d tuples with %d kinds of picture; the cover %d cells of %d tuples with %d" % (
        len(earlier), len({t for _, t in earlier}), len({s for s, _ in earlier}), len(new), len({t for _, t in new}), len({s for s, _ in new}))
    print(counts)
    assert earlier <= new, "%s; not in the cover: %s" % (counts, sorted(earlier - new)[:5])
    assert (len(earlier), len({t for _, t in earlier}), len(new)) == EARLIER, counts              # (the figures of DESIGN section 5)

