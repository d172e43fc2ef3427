"""The Intra 8x8 instances of the intra kernels are in the code object, without scratch; the instances every other batch launches
keep their 64 registers beside them (tests/test_kernel_resources.py holds them to that; this file only looks at the new pair)."""
import pytest

from p264decoder_amd import _native as N


def test_the_intra_8x8_kernels_are_in_the_code_object(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for name in ("k_intra_i8", "k_intra_sparse_i8"):
        assert name in res, sorted(res)
        r = res[name]
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 128, (name, r)            # sixteen wavefronts per workgroup: four per SIMD
    for name in ("k_intra", "k_intra_sparse"):
        assert name in res and res[name]["private_segment_fixed_size"] == 0
