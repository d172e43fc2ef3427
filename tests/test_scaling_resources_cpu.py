"""The kernels that a batch with a scaled picture launches are in the code object, spill no vector register and use no scratch;
the scaled intra instances stay within the 128 registers of four wavefronts per SIMD.  (tests/test_kernel_resources.py holds the
kernels of flat batches to their figures; this file only looks at the new ones.)"""
import pytest

from p264decoder_amd import _native as N

NEW = ("k_mc_sort_scaled", "k_mc_sort_scaled_p", "k_scaled_inter", "k_intra_scaled", "k_intra_sparse_scaled")


def test_the_scaling_kernels_are_in_the_code_object(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for name in NEW:
        assert name in res, sorted(res)
        r = res[name]
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    for name in ("k_intra_scaled", "k_intra_sparse_scaled"):
        assert res[name]["vgpr_count"] <= 128, (name, res[name])        # sixteen wavefronts per workgroup: four per SIMD
    assert res["k_scaled_inter"]["sgpr_spill_count"] == 0 and res["k_scaled_inter"]["vgpr_count"] <= 64, res["k_scaled_inter"]
