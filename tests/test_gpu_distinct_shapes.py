"""The forced launch shapes of tests/test_gpu_batch_shapes.py with distinct pictures.  That file gives every stream the same picture,
so a kernel that reads another picture's offsets, edge info, references or work lists there still writes the right bytes.  Here
every shape, odd-single count, edge-info mode and motion-compensation knob - and wavefronts that walk several work units - runs over three pools of CIF sources
(tests/distinct_pool.py): (a) Baseline P pictures - k_mc_sort, the fused edge info, k_deblock_bs<false>; (b) Main with B pictures -
k_mc_sort_b, k_mc_second, k_deblock_bs<true>; (c) pool (b) plus a source with explicit weights - k_mc_sort_b_wp, k_mc_wp - and over
two pools of High-profile sources of 11 x 9 macroblocks: (d) `high`, flat pictures with the 8x8 transform and Intra 8x8
macroblocks - k_t8x8 (13 workgroups per picture, the last with 3 macroblocks), k_intra_i8 / k_intra_sparse_i8 with 1 ... 16
wavefronts, k_deblock with the edge mask of the 8x8 transform at every multi-picture shape; (e) `scaled`, pictures with scaling
matrices (several tables) alternating with flat ones, one of them with explicit weights - k_mc_sort_scaled, k_mc_wp,
k_scaled_inter, k_intra_scaled / k_intra_sparse_scaled, a ScaleDev array that mixes the pictures' tables with the all-16 table;
(f) `scaled_plain`, pool (e) without the explicit weights - k_mc_sort_scaled_p and k_mc in the step of P pictures,
k_mc_sort_scaled, k_mc and k_mc_second in the steps with B pictures.  Batch
entry j decodes source j % K on a shuffled stream, so no deblocking workgroup holds two pictures of one source and no entry's
index is its stream.  Every stream of every step is checked, byte for byte; last_launch() shows that the forced shape and the
expected edge-info instance ran, and for (d) - (f) that the kernels they are there for were launched (k_t8x8, the Intra 8x8 and
the scaled instances: reported; which sort and which of k_mc / k_mc_wp: by the kinds of the batch's pictures, which every run checks)."""
import pytest

from tests import distinct_pool
from tests.hip_harness import reconstructor
from tests.stream_args import DISTINCT_STREAMS as S, LAUNCH_SHAPES as SHAPES, ODD, WAVES

pytestmark = pytest.mark.gpu

POOLS = {"p": (distinct_pool.POOL_P, 8), "b": (distinct_pool.POOL_B, 7), "wp": (distinct_pool.POOL_WP, 7),
         "high": (distinct_pool.POOL_HIGH, 7), "scaled": (distinct_pool.POOL_SCALED, 7), "scaled_plain": (distinct_pool.POOL_SCALED_PLAIN, 7)}
T8X8_WGS_PER_PICTURE = 13                # 99 macroblocks, 8 per workgroup of k_t8x8
FUSED = ["0", "1", "3", "16"]
MC_KNOBS = [("0", "4"), ("2", "7"), ("6", "200"), ("1", "16")]


@pytest.fixture(scope="module")
def pools(lib, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            specs, n = POOLS[name]
            cache[name] = distinct_pool.Pool(lib, specs, n, oracle=oracle)
        return cache[name]
    return get


# the kernels of the inter stage that the batches of a run over the pool must select in some step (launch_inter of p264hip.hip picks
# them from the batch's kinds; distinct_pool.expected_inter_instances restates that rule - the launch info does not name them)
INTER = {"p": {("k_mc_sort", "k_mc")},
         "b": {("k_mc_sort", "k_mc"), ("k_mc_sort_b", "k_mc", "k_mc_second")},
         "wp": {("k_mc_sort_wp", "k_mc_wp"), ("k_mc_sort_b_wp", "k_mc_wp", "k_mc_second")},
         "high": {("k_mc_sort", "k_mc"), ("k_mc_sort_b", "k_mc", "k_mc_second")},
         "scaled": {("k_mc_sort_scaled", "k_mc_wp"), ("k_mc_sort_scaled", "k_mc_wp", "k_mc_second")},
         "scaled_plain": {("k_mc_sort_scaled_p", "k_mc"), ("k_mc_sort_scaled", "k_mc", "k_mc_second")}}


def content_launches(pool_name, pool, t, li, pics):
    """what the batch's content launched.  Behind the IDR step `high` ran k_t8x8 over every picture and the Intra 8x8 intra instances, and no scaled instance; `scaled`
    and `scaled_plain` ran the scaled instances (k_scaled_inter in k_t8x8's place, the scaled intra instances with Intra 8x8) with
    as many scaled entries as the batch holds"""
    if t == 0:
        return
    if pool_name == "high":
        assert (li["t8x8_wgs"], li["intra_i8"], li["scaled_pictures"]) == (T8X8_WGS_PER_PICTURE * S, 1, 0), (t, li)
    elif pool_name in ("scaled", "scaled_plain"):
        scaled_entries = sum(bool(int(pics[j % pool.K].desc.scaling_lists)) for j in range(S))
        assert 0 < scaled_entries < S and (li["scaled_pictures"], li["t8x8_wgs"], li["intra_i8"]) == (scaled_entries, 0, 1), (t, scaled_entries, li)


def run(lib, pool_name, pool, seed, on_step):
    seen = set()

    def step(t, li, pics):
        seen.add(distinct_pool.expected_inter_instances([pics[j % pool.K] for j in range(S)]))      # (of the batch as uploaded)
        content_launches(pool_name, pool, t, li, pics)
        on_step(t, li, pics)
    with reconstructor(lib, pool.mb_w, pool.mb_h, n_streams=S, slots=pool.slots, max_pictures=pool.K) as hip:
        pool.run(hip, S, seed, step)
    assert seen >= INTER[pool_name] | {()}, (pool_name, seen)


@pytest.mark.parametrize("rb,per_wg,intra_waves", SHAPES)
@pytest.mark.parametrize("pool_name", list(POOLS))
def test_workgroup_shapes_with_distinct_pictures(lib, pools, pool_name, rb, per_wg, intra_waves, monkeypatch):
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", rb)
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)
    monkeypatch.setenv("P264AMD_INTRA_WAVES", intra_waves)
    pool = pools(pool_name)

    def on_step(t, li, pics):
        assert (li["pictures"], li["deblock_rb_log2"], li["deblock_pics_per_wg"], li["intra_waves"], li["deblock_odd_single"]) == \
            (S, int(rb), int(per_wg), int(intra_waves), 0), li
        assert li["edge_info_fused"] == distinct_pool.expected_edge_info_fused(pics), (t, li)
    run(lib, pool_name, pool, int(rb) * 1000 + int(per_wg) * 10 + int(intra_waves), on_step)


@pytest.mark.parametrize("rb,per_wg,waves", WAVES)
@pytest.mark.parametrize("pool_name", list(POOLS))
def test_several_units_per_wavefront_with_distinct_pictures(lib, pools, pool_name, rb, per_wg, waves, monkeypatch):
    """fewer k_deblock wavefronts than work units (P264AMD_DEBLOCK_WAVES): a wavefront walks several units, and with a wavefront
    count that does not divide the groups its octets move to other pictures of the workgroup - whose QPs may be the same and whose
    loop-filter offsets are not (the octet's expanded alpha / beta belong to one unit)"""
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", rb)
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)
    monkeypatch.setenv("P264AMD_DEBLOCK_WAVES", waves)
    pool = pools(pool_name)

    def on_step(t, li, pics):
        assert (li["deblock_rb_log2"], li["deblock_pics_per_wg"], li["deblock_waves"], li["deblock_odd_single"]) == (int(rb), int(per_wg), int(waves), 0), li
    run(lib, pool_name, pool, 300 + int(per_wg) * 10 + int(waves), on_step)


@pytest.mark.parametrize("per_wg", ODD)
@pytest.mark.parametrize("pool_name", list(POOLS))
def test_odd_picture_counts_with_distinct_pictures(lib, pools, pool_name, per_wg, monkeypatch):
    """pairs in bands of 4 rows and the last picture of the workgroup alone in bands of 8 (odd_single)"""
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", "2")
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)
    monkeypatch.setenv("P264AMD_DEBLOCK_ODD_SINGLE", "1")
    pool = pools(pool_name)

    def on_step(t, li, pics):
        assert (li["deblock_odd_single"], li["deblock_rb_log2"], li["deblock_pics_per_wg"]) == (1, 2, int(per_wg)), li
        assert li["edge_info_fused"] == distinct_pool.expected_edge_info_fused(pics), (t, li)
    run(lib, pool_name, pool, 500 + int(per_wg), on_step)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("pool_name", list(POOLS))
def test_edge_info_modes_with_distinct_pictures(lib, pools, pool_name, fused, monkeypatch):
    """the edge info in its own k_deblock_bs launch or in 1 / 3 / 16 extra workgroups per picture of k_intra_sparse (steps of
    unweighted P pictures only; any I, B or weighted picture, any picture with the 8x8 transform or scaling lists takes the own launch)"""
    monkeypatch.setenv("P264AMD_BS_FUSED", fused)
    pool = pools(pool_name)
    kinds = set()

    def on_step(t, li, pics):
        want = distinct_pool.expected_edge_info_fused(pics, fused)
        assert li["edge_info_fused"] == want, (t, li)
        kinds.add(want)
    run(lib, pool_name, pool, 700 + int(fused), on_step)
    assert kinds == ({0, int(fused)} if pool_name in ("p", "b") else {0}), kinds       # (the others: never a step of plain P pictures)


@pytest.mark.parametrize("band_log2,wgs", MC_KNOBS)
@pytest.mark.parametrize("pool_name", list(POOLS))
def test_mc_launch_knobs_with_distinct_pictures(lib, pools, pool_name, band_log2, wgs, monkeypatch):
    """locality bands of 1 / 4 / 64 macroblock rows, 4 ... 200 motion-compensation workgroups per picture (capped by the chunks
    there can be): for pools (b) and (c) the first runs of k_mc_sort_b, k_mc_second and k_mc_wp under these shapes"""
    monkeypatch.setenv("P264AMD_MC_BAND_LOG2", band_log2)
    monkeypatch.setenv("P264AMD_MC_WGS_PER_PIC", wgs)
    pool = pools(pool_name)

    def on_step(t, li, pics):
        if t == 0:                                           # IDR pictures only: no inter launch
            assert li["mc_wgs_per_picture"] == 0, li
        elif int(wgs) <= 7:
            assert li["mc_wgs_per_picture"] == int(wgs), (t, li)
        else:
            assert 4 <= li["mc_wgs_per_picture"] <= int(wgs), (t, li)
    run(lib, pool_name, pool, 900 + int(band_log2) * 7 + int(wgs), on_step)
