"""tests/deblock_checker.py - the loop filter typed from H.264 8.7 - against everything else that claims to know the filter (CPU):

* the reference's recorded answers: all 160 pictures of kat_deblock_frame.npz, which anchors the checker to the real reference
  where the reference goes (P pictures, one list, no slices);
* oracle_deblock_picture, byte for byte, on the pictures of every seam-level family of the GPU suites (drawn by their own
  helpers), on the directed stimulus pictures of tests/deblock_stim.py, and on families whose lists hold one frame at several
  indices.  On the parent of the commit that brought this file the oracle compared list INDICES in P pictures and the
  duplicated-P family failed (8.7.2.1 says "different reference pictures");
* the census: over the stimulus set every cell of deblock_checker.all_cells() - (plane, strength, branch) x edge direction x line
  parity x macroblock / inner edge - occurs at least 8 times.  8 is a condition on the stimulus, not a measurement: no cell may
  rest on one line.  tests/test_gpu_deblock_spec.py compares the kernels with the checker on the same pictures and relies on it;
* ValueError for every `edges` pattern the seam leaves undefined."""
import collections
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import deblock_checker as dc
from tests import deblock_stim, intra_checker, kat_seam, oracle_bind, seam_fuzz
from tests import intra_avail_stim as t_intra
from tests import ipcm_seam_stim as t_ipcm
from tests import wp_seam_stim as t_wp
from tests.conftest import GOLDEN
from tests.stream_args import SEAM_CONFIGS

# one frame at several indices of a list (what reordering commands that name a picture twice, or a list longer than the frame
# store, produce): unweighted P - also with indices past the list - and B with a frame twice in a list and in both lists
DUP_FAMILIES = [
    ("p_dup", 9, 7, 6, dict(level_style="small", qp_mode="two", n_ref=3, slots=4, dup_refs=True, mv_range=6)),
    ("p_dup_past_list", 9, 7, 6, dict(level_style="small", qp_mode="two", n_ref=3, slots=4, dup_refs=True, mv_range=6, past_list=0.3)),
    ("p_dup_two_slots", 10, 6, 5, dict(level_style="small", qp_mode="random", n_ref=4, slots=3, dup_refs=True, mv_range=6, slices=2)),
    ("b_dup_both_lists", 9, 7, 6, dict(level_style="small", qp_mode="two", n_ref=3, n_ref_l1=3, slots=3, b_picture=True, dup_refs=True,
                                        mv_range=6, mirror_l1=0.5)),
]


def dup_family_inputs(name, mb_w, mb_h, n_pics, kw):
    """a family's starting frames (smooth: the filter's conditions hold), then its pictures, lazily (picture 2 is an I picture)"""
    rng = np.random.default_rng(sum(map(ord, name)) * 7817)
    yield [seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth") for _ in range(kw["slots"])]
    for i in range(n_pics):
        yield seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=(i != 2), dst_slot=i % kw["slots"], **kw)


def differing(a, b):
    return sum(int((x != y).sum()) for x, y in zip(a, b))


def both_filters(oracle, store, pic, census=None):
    """the unfiltered picture lies in its frame of the store: the checker filters a copy, the oracle the frame (where the next
    picture finds it); returns the samples that differ"""
    mine = [a.copy() for a in store[pic.desc.dst_slot]]
    if pic.desc.deblock:
        dc.deblock(pic, mine, census)
        oracle.oracle_deblock_picture(C.byref(pic.desc), store.ptrs)
    return differing(mine, store[pic.desc.dst_slot])


def test_tables():
    """spot values of tables 8-15, 8-16, 8-17 a reader can hold against the standard"""
    assert dc.ALPHA[15:18] == [0, 4, 4] and dc.ALPHA[51] == 255 and dc.ALPHA[36] == 50
    assert dc.BETA[15:17] == [0, 2] and dc.BETA[51] == 18 and dc.BETA[26] == 6
    assert dc.TC0[16] == (0, 0, 0) and dc.TC0[17] == (0, 0, 1) and dc.TC0[21] == (0, 1, 1) and dc.TC0[23] == (1, 1, 1) and dc.TC0[51] == (13, 17, 25)
    assert dc.CHROMA_QP[29:35] == [29, 29, 30, 31, 32, 32] and dc.CHROMA_QP[51] == 39
    assert all(a <= b for a, b in zip(dc.ALPHA, dc.ALPHA[1:])) and all(a <= b for t in zip(*dc.TC0) for a, b in zip(t, t[1:]))


def test_hand_computed_lines():
    """8.7.2.3 / 8.7.2.4 on lines worked by hand"""
    # indexA 36: alpha 50, tc0 (bS 1) = 2; indexB 34: beta 10.  ap = 2 < 10, aq = 1 < 10: tc = 4; delta = (4 * 10 + (58 - 71) + 4) >> 3 = 3
    assert dc.filter_line([60, 62, 58, 60, 70, 71, 69, 70], False, 1, 36, 50, 10) == [60, 62, 60, 63, 67, 69, 69, 70]
    # the same chroma line: tc = 3, delta = 3
    assert dc.filter_line([58, 60, 70, 71], True, 1, 36, 50, 10) == [58, 63, 67, 71]
    # strength 4, |p0 - q0| = 4 < (50 >> 2) + 2, both sides smooth: the long filters
    assert dc.filter_line([100, 100, 100, 100, 104, 104, 104, 104], False, 4, 36, 50, 10) == [100, 101, 101, 102, 103, 103, 104, 104]
    # strength 4, |p0 - q0| = 20 >= 14: the short filter on both sides
    assert dc.filter_line([100, 100, 100, 100, 120, 120, 120, 120], False, 4, 36, 50, 10) == [100, 100, 100, 105, 115, 120, 120, 120]
    # |p0 - q0| = alpha: untouched
    s = [0, 0, 0, 0, 50, 50, 50, 50]
    assert dc.filter_line(s, False, 2, 36, 50, 10) is s


def test_checker_equals_the_references_recorded_answers():
    kat = np.load(GOLDEN + "/kat_deblock_frame.npz")
    n = len(kat["dbf_y"])
    assert n == 160
    for i in range(n):
        pic, ref, want = kat_seam.deblock_frame_case(kat, i)
        mine = [kat["dbf_y"][i].copy(), kat["dbf_u"][i].copy(), kat["dbf_v"][i].copy()]
        dc.deblock(pic, mine)
        assert differing(mine, want) == 0, "case %d: %d samples differ from the reference's filtered picture" % (i, differing(mine, want))


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", SEAM_CONFIGS, ids=[c[0] for c in SEAM_CONFIGS])
def test_checker_equals_oracle_on_seam_fuzz(oracle, name, mb_w, mb_h, n_pics, kw):
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    slots = kw["slots"]
    store = oracle_bind.FrameStore(mb_w, mb_h, slots)
    for s in range(slots):
        for dst, src in zip(store[s], seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if "smooth" in name else "noise")):
            dst[:] = src
    for i in range(n_pics):
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=(i != 2), dst_slot=i % slots, **kw)
        oracle_bind.reconstruct(oracle, store, pic, deblock=False)
        assert both_filters(oracle, store, pic) == 0, "%s picture %d" % (name, i)


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", DUP_FAMILIES, ids=[c[0] for c in DUP_FAMILIES])
def test_checker_equals_oracle_with_one_frame_at_several_indices(oracle, name, mb_w, mb_h, n_pics, kw):
    """(the duplicated-P families fail against an oracle that compares a P picture's list indices)"""
    inputs = dup_family_inputs(name, mb_w, mb_h, n_pics, kw)
    store = oracle_bind.FrameStore(mb_w, mb_h, kw["slots"])
    for s, f in enumerate(next(inputs)):
        for dst, src in zip(store[s], f):
            dst[:] = src
    twice = 0
    for i, pic in enumerate(inputs):
        d = pic.desc
        twice += len(set(d.ref_slot[:d.n_ref])) < d.n_ref
        oracle_bind.reconstruct(oracle, store, pic, deblock=False)
        assert both_filters(oracle, store, pic) == 0, "%s picture %d" % (name, i)
    assert twice >= n_pics - 1


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", t_wp.CONFIGS, ids=[c[0] for c in t_wp.CONFIGS])
def test_checker_equals_oracle_on_wp_seam_fuzz(oracle, name, mb_w, mb_h, n_pics, kw):
    chk = intra_checker.IntraChecker(oracle, mb_w, mb_h, kw["slots"])
    inputs = t_wp.config_inputs(name, mb_w, mb_h, n_pics, kw)
    for s, f in enumerate(next(inputs)):
        for dst, src in zip(chk.store[s], f):
            dst[:] = src
    for i, pic in enumerate(inputs):
        chk.nodeblock(pic)
        assert both_filters(oracle, chk.store, pic) == 0, "%s picture %d" % (name, i)


@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(t_ipcm.CONFIGS))
def test_checker_equals_oracle_on_ipcm_seam_fuzz(oracle, name, with_i):
    mb_w, mb_h = t_ipcm.CONFIGS[name][:2]
    batch, seen = t_ipcm.prepare(oracle, name, with_i)
    for s, (pic, refs, want) in enumerate(batch):
        chk = intra_checker.IntraChecker(oracle, mb_w, mb_h, t_ipcm.SLOTS)
        for slot in range(t_ipcm.DST):
            for dst, src in zip(chk.store[slot], refs[slot]):
                dst[:] = src
        chk.nodeblock(pic)
        assert both_filters(oracle, chk.store, pic) == 0, "%s stream %d" % (name, s)


@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(t_intra.FAMILIES))
def test_checker_equals_oracle_on_intra_availability(oracle, name, with_i):
    mb_w, mb_h = t_intra.FAMILIES[name][:2]
    for s, (pic, f, target) in enumerate(t_intra.draw(name, with_i)):
        chk = intra_checker.IntraChecker(oracle, mb_w, mb_h, t_intra.SLOTS)
        for slot in range(t_intra.DST):
            for dst, src in zip(chk.store[slot], f):
                dst[:] = src
        chk.nodeblock(pic)
        assert both_filters(oracle, chk.store, pic) == 0, "%s stream %d" % (name, s)


# ---- the stimulus set ----
@pytest.fixture(scope="module")
def stimulus(oracle):
    """[(Stim, the checker's filtered planes)] and the census of the checker's run over all of them"""
    census = collections.Counter()
    out = []
    for st in deblock_stim.stimulus_set():
        out.append((st, deblock_stim.expected(oracle, st, census)))
    return out, census


def test_checker_equals_oracle_on_the_stimulus(oracle, stimulus):
    for st, want in stimulus[0]:
        store = deblock_stim.store_of(st)
        oracle_bind.reconstruct(oracle, store, st.pic)
        assert differing(want, store[st.pic.desc.dst_slot]) == 0, st.name


def test_every_cell_of_the_census_occurs_8_times(stimulus):
    deblock_stim.check_census(stimulus[1])


def test_the_stimulus_sweeps_what_it_says(stimulus):
    """indexA over its range with the thresholds' corners, offsets odd and even over -12 .. 12, both plane kinds, QP means"""
    ia, offs, cqos, mean = set(), set(), set(), 0
    for st, _ in stimulus[0]:
        d, rec = st.pic.desc, st.pic.rec
        offs |= {int(d.alpha_c0_offset), int(d.beta_offset)}
        cqos.add(int(d.chroma_qp_offset))
        qp = rec["qp"].reshape(st.pic.mb_h, st.pic.mb_w).astype(int)
        mean += int(((qp[:, 1:] - qp[:, :-1]) % 2 != 0).sum() + ((qp[1:] - qp[:-1]) % 2 != 0).sum())
        for q in set(qp.reshape(-1).tolist()):
            ia.add(dc.thresholds(q, d.alpha_c0_offset, d.beta_offset)[0])
            ia.add(dc.thresholds(dc.chroma_qp_av(q, q, d.chroma_qp_offset), d.alpha_c0_offset, d.beta_offset)[0])
    assert {0, 15, 16, 17, 23, 24, 51} <= ia and len(ia) >= 40, sorted(ia)
    assert {-12, 12} <= offs and any(o & 1 for o in offs) and any(not o & 1 for o in offs), sorted(offs)
    assert min(cqos) <= -8 and max(cqos) >= 8, sorted(cqos)
    assert mean > 0, "no edge between QPs whose mean rounds"
    assert all(st.pic.mb_w >= 6 and st.pic.mb_h >= 6 and max(st.pic.mb_w, st.pic.mb_h) >= 9 for st, _ in stimulus[0])


# ---- what the seam leaves undefined ----
def _plain_picture():
    rng = np.random.default_rng(5)
    pic = seam_fuzz.make_picture(rng, 4, 3, n_ref=1, slots=2, qp_mode=30)
    planes = seam_fuzz.random_frame(rng, 4, 3, "smooth")
    return pic, planes


@pytest.mark.parametrize("mb,flags", [(4, N.EDGE_LEFT | N.EDGE_INNER), (2, N.EDGE_TOP | N.EDGE_INNER), (5, N.EDGE_LEFT), (6, N.EDGE_TOP),
                                      (9, N.EDGE_LEFT | N.EDGE_TOP)],
                         ids=["left_at_column_0", "top_at_row_0", "left_without_inner", "top_without_inner", "both_without_inner"])
def test_malformed_edges_raise(mb, flags):
    pic, planes = _plain_picture()
    dc.deblock(pic, [p.copy() for p in planes])                 # (well-formed as drawn)
    pic.rec["edges"][mb] = flags
    before = [p.copy() for p in planes]
    with pytest.raises(ValueError):
        dc.deblock(pic, planes)
    assert differing(before, planes) == 0, "the checker wrote before it refused"
