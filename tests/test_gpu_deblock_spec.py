"""The loop filter's kernels (edge info: the fused role of k_intra_sparse, k_deblock_bs<false>, k_deblock_bs<true>; samples:
k_deblock) against tests/deblock_checker.py - the filter typed from H.264 8.7, not the oracle's - on the directed pictures of
tests/deblock_stim.py and on pictures whose lists hold one frame at several indices.  Prediction and residual come from the
existing roads (oracle_reconstruct_nodeblock); only the last step is the checker's.  Bytes of all three planes, every picture.

Batches: one stream per picture, every stream a DIFFERENT picture with its own offsets; per edge direction of the stimulus (9 x 6
macroblocks for vertical edges, 6 x 9 transposed) once through each edge-info instance, once with an odd picture count per
workgroup in bands of 4 rows and once with fewer wavefronts than work units - the pictures are taller than a band, so their lines
cross band seams - and one 1080p picture of stimulus rows repeated.  What the comparison covers is the census of the checker's
own run (test_the_census_behind_this_file; the CPU twin is tests/test_deblock_checker_cpu.py).

The duplicated-P cases are the ones a kernel that compares list indices in unweighted P pictures (the parent's kernel_deblock.h)
gets wrong."""
import collections

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import deblock_checker as dc
from tests import deblock_stim, oracle_bind, seam_fuzz
from tests.hip_harness import compare, load_frames, reconstructor

pytestmark = pytest.mark.gpu

SLOTS = 3                    # every picture writes slot 0 and reads slots 1, 2
GEOMS = {"v": (deblock_stim.MB_W, deblock_stim.MB_H), "h": (deblock_stim.MB_H, deblock_stim.MB_W)}
# pictures whose lists hold one frame twice (slots [1, 1, 2]; B: list 1 = [2, 2, 1], so every frame is in both lists as well)
DUP_KINDS = {
    "p_dup": dict(n_ref=3, dup_refs=True, mv_range=6),
    "p_dup_sliced": dict(n_ref=3, dup_refs=True, mv_range=6, slices=3, qp_mode="two"),
    "p_dup_past_list": dict(n_ref=3, dup_refs=True, mv_range=6, past_list=0.3),
    "b_dup": dict(n_ref=3, n_ref_l1=3, dup_refs=True, mv_range=6, b_picture=True, mirror_l1=0.5),
}


def dup_pictures(oracle, direction):
    """[Stim] of DUP_KINDS at a geometry: smooth reference frames (different per slot), the checker's expectation alongside"""
    mb_w, mb_h = GEOMS[direction]
    out = []
    for name, kw in DUP_KINDS.items():
        rng = np.random.default_rng(sum(map(ord, name + direction)) * 7723)
        frames = {slot: seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth") for slot in (1, 2)}
        k = dict(level_style="small", qp_mode="random", intra_share=0.1)
        k.update(kw)
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, slots=SLOTS, dst_slot=0, **k)
        d = pic.desc
        assert len(set(d.ref_slot[:d.n_ref])) < d.n_ref
        store = oracle_bind.FrameStore(mb_w, mb_h, SLOTS)
        for slot, f in frames.items():
            for dst, src in zip(store[slot], f):
                dst[:] = src
        want = [a.copy() for a in oracle_bind.reconstruct(oracle, store, pic, deblock=False)]
        dc.deblock(pic, want)
        out.append((name, pic, frames, want))
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """per direction: [(name, picture, {slot: frame}, the checker's planes)] - the stimulus pictures, then the duplicated lists;
    and the census of the stimulus"""
    census = collections.Counter()
    per = {"v": [], "h": []}
    for st in deblock_stim.stimulus_set():
        direction = "h" if "_h_" in st.name else "v"
        assert (st.pic.mb_w, st.pic.mb_h) == GEOMS[direction]
        per[direction].append((st.name, st.pic, {slot: st.frame for slot in st.ref_slots}, deblock_stim.expected(oracle, st, census)))
    n_stim = {k: len(v) for k, v in per.items()}
    for direction in per:
        per[direction] += dup_pictures(oracle, direction)
    return per, n_stim, census


def run_batch(lib, direction, batch, extra=None):
    """the pictures of `batch` in one p264hip_reconstruct call, one stream each (extra: a picture that only shapes the batch, on
    the last stream, unchecked); compares every picture; returns the launch info"""
    mb_w, mb_h = GEOMS[direction]
    pics = [b[1] for b in batch] + ([extra] if extra is not None else [])
    n = len(pics)
    with reconstructor(lib, mb_w, mb_h, n_streams=n, slots=SLOTS, max_pictures=n) as hip:
        for s, (name, pic, frames, want) in enumerate(batch):
            load_frames(hip, s, frames)
        hip.upload(0, pics)
        hip.reconstruct(list(range(n)), list(range(n)))
        li = hip.last_launch()
        assert li["pictures"] == n
        for s, (name, pic, frames, want) in enumerate(batch):
            compare(hip.read_frame(s, 0), want, "%s (stream %d of %d)" % (name, s, n), pic)
    return li


def is_plain_p(pic):
    d = pic.desc
    return d.slice_type == N.SLICE_P and not d.explicit_wp and len(set(d.ref_slot[:d.n_ref])) == d.n_ref


@pytest.mark.parametrize("direction", ["v", "h"])
def test_stimulus_through_the_fused_edge_info(lib, cases, direction):
    """a batch of unweighted P pictures whose lists name every frame once: the edge info comes from k_intra_sparse"""
    per, n_stim, _ = cases
    batch = per[direction][:n_stim[direction]]
    assert all(is_plain_p(b[1]) for b in batch) and len({(b[1].desc.alpha_c0_offset, b[1].desc.beta_offset) for b in batch}) > 6
    li = run_batch(lib, direction, batch)
    assert li["edge_info_fused"] > 0, li


@pytest.mark.parametrize("how", ["fused_off", "with_i_picture"])
@pytest.mark.parametrize("direction", ["v", "h"])
def test_stimulus_through_the_one_list_edge_info_kernel(lib, cases, direction, how, monkeypatch):
    """k_deblock_bs<false>: the fused road switched off, or an I picture in the batch (dense k_intra carries no edge-info role)"""
    per, n_stim, _ = cases
    batch = per[direction][:n_stim[direction]]
    extra = None
    if how == "fused_off":
        monkeypatch.setenv("P264AMD_BS_FUSED", "0")
    else:
        extra = seam_fuzz.make_picture(np.random.default_rng(3), *GEOMS[direction], p_picture=False, slots=SLOTS, dst_slot=0)
    li = run_batch(lib, direction, batch, extra)
    assert li["edge_info_fused"] == 0, li


@pytest.mark.parametrize("direction", ["v", "h"])
def test_everything_through_the_two_list_edge_info_kernel(lib, cases, direction):
    """a B picture in the batch: k_deblock_bs<true> for every picture - the stimulus and the duplicated lists, P and B"""
    per, _, _ = cases
    batch = per[direction]
    assert any(b[1].desc.slice_type == N.SLICE_B for b in batch)
    li = run_batch(lib, direction, batch)
    assert li["edge_info_fused"] == 0, li


@pytest.mark.parametrize("direction", ["v", "h"])
def test_unweighted_p_with_one_frame_twice_compares_pictures(lib, cases, direction):
    """batches of unweighted P pictures only, some with a frame at two indices: such a batch leaves the fused road (whose test goes
    by index) for k_deblock_bs<true>, and every picture - duplicated list or not - is the checker's"""
    per, n_stim, _ = cases
    dups = [b for b in per[direction][n_stim[direction]:] if b[1].desc.slice_type == N.SLICE_P]
    assert len(dups) == 3 and not any(is_plain_p(b[1]) for b in dups)
    li = run_batch(lib, direction, dups)
    assert li["edge_info_fused"] == 0, li
    li = run_batch(lib, direction, [dups[0]])
    assert li["edge_info_fused"] == 0, li
    li = run_batch(lib, direction, per[direction][:5] + dups[1:])
    assert li["edge_info_fused"] == 0, li


@pytest.mark.parametrize("direction", ["v", "h"])
def test_odd_picture_count_per_workgroup_in_bands_of_4_rows(lib, cases, direction, monkeypatch):
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", "2")
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", "3")
    monkeypatch.setenv("P264AMD_DEBLOCK_ODD_SINGLE", "1")
    per, _, _ = cases
    assert GEOMS[direction][1] > 4                       # lines cross the seam between a picture's bands
    li = run_batch(lib, direction, per[direction])
    assert (li["deblock_odd_single"], li["deblock_rb_log2"], li["deblock_pics_per_wg"]) == (1, 2, 3), li


@pytest.mark.parametrize("direction,rb,per_wg,waves", [("v", "2", "4", "3"), ("h", "2", "4", "3"), ("h", "3", "3", "2")])
def test_fewer_wavefronts_than_units(lib, cases, direction, rb, per_wg, waves, monkeypatch):
    """a wavefront walks several units: its octets move on to other pictures, whose offsets differ"""
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", rb)
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)
    monkeypatch.setenv("P264AMD_DEBLOCK_WAVES", waves)
    per, n_stim, _ = cases
    assert GEOMS[direction][1] > 1 << int(rb)
    li = run_batch(lib, direction, per[direction][:n_stim[direction]])
    assert (li["deblock_rb_log2"], li["deblock_pics_per_wg"], li["deblock_waves"], li["deblock_odd_single"]) == (int(rb), int(per_wg), int(waves), 0), li
    assert li["edge_info_fused"] > 0, li


def test_1080p_of_stimulus_rows_repeated(lib, oracle):
    """120 x 68 macroblocks tiled from a picture of strengths 3 / 4 (its inter rows carry 0 and 4): 17 bands of 4 rows or 9 of 8, 120
    columns of lag, one stream by p264hip_submit"""
    st = next(s for s in deblock_stim.stimulus_set(rounds=1) if s.name.startswith("intra_v"))
    big = deblock_stim.tiled_1080p(st)
    census = collections.Counter()
    want = deblock_stim.expected(oracle, big, census)
    assert sum(n for c, n in census.items() if c[1] == 4) > 20000 and sum(n for c, n in census.items() if c[1] == 3) > 20000
    with reconstructor(lib, big.pic.mb_w, big.pic.mb_h, n_streams=1, slots=SLOTS, max_pictures=1) as hip:
        for slot in big.ref_slots:
            hip.write_frame(0, slot, *big.frame)
        hip.submit(0, big.pic)
        compare(hip.read_frame(0, 0), want, big.name, big.pic)


def test_the_census_behind_this_file(cases):
    """what the comparisons above covered: every cell of the checker's class list at least 8 times over the stimulus pictures"""
    deblock_stim.check_census(cases[2])
