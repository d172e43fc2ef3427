"""The two batch shapes the benchmark runs at size, with distinct pictures: the bench's own batch (8 x compute units streams of
1080p IDR + 3 P pictures) and BASELINE config 4's (4 x compute units streams of 1080p Main, I P B B P B B).  The tests of
tests/test_gpu_synth.py and tests/test_gpu_main_profile.py give every stream the same picture or decode one picture per call; here
batch entry j decodes source j % K (K = 10 and 9, more than the 8 and 4 pictures of a k_deblock workgroup) on a shuffled stream
(tests/distinct_pool.py).  Every stream of every step is checked: pinned sources against their committed reference (oracle)
hashes, the others against the oracle."""
import pytest

from p264decoder_amd import _native as N
from tests import distinct_pool
from tests.hip_harness import reconstructor

pytestmark = pytest.mark.gpu


def compute_units(lib, pool):
    with reconstructor(lib, pool.mb_w, pool.mb_h, n_streams=1, slots=pool.slots, max_pictures=1) as probe:
        return probe.last_launch()["compute_units"]


def test_the_bench_s_own_batch_with_distinct_sources(lib, oracle):
    """8 x CUs streams (2048 on an MI355X): 8 pictures per k_deblock workgroup in bands of four rows, 48 k_mc workgroups per
    picture, 4 intra wavefronts, the edge info inside the intra launch of the P steps - what test_the_bench_s_own_batch_against_
    reference_hashes asserts, with ten different sources in every run of ten entries.  cfg3_1080p_allp, cfg3_1080p_ip,
    cfg3_1080p_ip_l32 and qpd_1080p are checked against the real reference decoder's hashes."""
    pool = distinct_pool.Pool(lib, distinct_pool.POOL_BENCH, 4, oracle=oracle)
    n_cu = compute_units(lib, pool)
    S = 8 * n_cu
    assert pool.K > 8

    def on_step(t, li, pics):
        assert li["pictures"] == S and li["deblock_pics_per_wg"] == 8 and li["deblock_rb_log2"] == 2 and li["deblock_wgs"] == n_cu and li["intra_waves"] == 4, li
        if all(p.desc.slice_type == N.SLICE_P for p in pics):
            assert li["mc_wgs_per_picture"] == 48 and li["edge_info_fused"] == 1, li
    with reconstructor(lib, pool.mb_w, pool.mb_h, n_streams=S, slots=pool.slots, max_pictures=pool.K) as hip:
        pool.run(hip, S, 2048, on_step)


def test_config4_batch_with_distinct_sources(lib, oracle):
    """4 x CUs streams (1024 on an MI355X) of 1080p Main, no explicit weights: exactly config 4's kernels - k_mc_sort_b, k_mc,
    k_mc_second with 48 workgroups per picture, 4 intra wavefronts, 4 pictures per k_deblock workgroup, k_deblock_bs<true>.  Eight
    sources put two B pictures between reference pictures, one puts one, so steps 3 - 5 mix P and B pictures.
    main_1080p_cabac_ipb (config 4's own stream) is checked against its committed oracle hashes."""
    pool = distinct_pool.Pool(lib, distinct_pool.POOL_CFG4, 7, oracle=oracle)
    n_cu = compute_units(lib, pool)
    S = 4 * n_cu
    assert pool.K > 4 and not any(p.desc.explicit_wp for s in pool.sources for p in s.pics)
    kinds = []

    def on_step(t, li, pics):
        types = {p.desc.slice_type for p in pics}
        assert li["pictures"] == S and li["intra_waves"] == 4 and li["deblock_pics_per_wg"] == 4, (t, li)
        if types == {N.SLICE_I}:
            assert li["mc_wgs_per_picture"] == 0 and li["edge_info_fused"] == 0, (t, li)      # IDR step: no inter launch
        else:
            assert li["mc_wgs_per_picture"] == 48, (t, li)
            # a B picture in the step: the B instances and k_deblock_bs<true>; P pictures only: the fused edge info
            assert li["edge_info_fused"] == (0 if N.SLICE_B in types else 1), (t, li)
        kinds.append(types)
    with reconstructor(lib, pool.mb_w, pool.mb_h, n_streams=S, slots=pool.slots, max_pictures=pool.K) as hip:
        pool.run(hip, S, 1024, on_step)
    assert {N.SLICE_P} in kinds and {N.SLICE_B} in kinds and kinds.count({N.SLICE_P, N.SLICE_B}) == 3, kinds
