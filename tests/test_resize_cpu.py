"""The host side of the resized device export (include/p264hip.h: p264hip_resize_t), no GPU: the tap positions against the formula in
exact fractions, the numpy model of tests/resize_checker.py against float64 bilinear, the layout and the refusals of
p264hip_resize_frame_bytes / p264hip_resize_check, the ctypes mirror, and the kernels in the code object."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import export_checker as X
from tests import resize_checker as R

EINVAL = -1
PAIRS = [(2, 2), (2, 16384), (16384, 2), (80, 80), (80, 40), (48, 98), (62, 34), (1080, 224), (1920, 640), (30, 2)]
KERNELS = ("k_resize_i420", "k_resize_nv12", "k_resize_rgb24_u8", "k_resize_rgb24_f16", "k_resize_rgb24_f32",
           "k_resize_rgbp_u8", "k_resize_rgbp_f16", "k_resize_rgbp_f32")


def desc(fmt="rgbp", size=(34, 18), crop=(0, 0, 80, 48), **kw):
    return N.resize_desc(fmt, size, crop, None, **kw)


@pytest.mark.parametrize("S,D", PAIRS)
def test_taps_are_the_formula_in_exact_fractions(lib, S, D):
    pos = (C.c_int32 * D)()
    assert lib.p264hip_resize_taps(S, D, pos) == 0
    got = np.ctypeslib.as_array(pos)
    step = max(1, D // 997)                                  # (every index of the short axes, a thousand of the long one, both ends)
    for d in sorted(set(range(0, D, step)) | {0, 1, D - 2, D - 1} & set(range(D))):
        want = min(max(math.floor(Fraction((2 * d + 1) * S * 256 + D, 2 * D)) - 128, 0), (S - 1) * 256)
        assert got[d] == want, (S, D, d)
    assert np.array_equal(got, R.taps(S, D))                 # ... and the checker's, at every index
    assert got.min() >= 0 and got.max() <= (S - 1) * 256


def test_taps_refusals(lib):
    pos = (C.c_int32 * 4)()
    assert lib.p264hip_resize_taps(2, 4, pos) == 0
    for S, D, p in ((0, 4, pos), (2, 0, pos), (-1, 4, pos), (2, -1, pos), (2, 4, None), ((1 << 20) + 1, 4, pos)):
        assert lib.p264hip_resize_taps(S, D, p) == EINVAL


def test_the_model_is_within_1_of_float64_bilinear():
    g = np.random.default_rng(2646)
    peak = 0
    for sw, sh in ((80, 48), (62, 30), (2, 2), (48, 22), (40, 24)):
        yy, xx = np.mgrid[0:sh, 0:sw]
        for src in (g.integers(0, 256, (sh, sw), np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8), np.full((sh, sw), 255, np.uint8)):
            for W, H in ((sw, sh), (sw // 2, sh // 2), (34, 18), (162, 98), (2, 2), (6, 70), (224, 224), (1, 1)):
                if W < 1 or H < 1:
                    continue
                got, top = R.resize_plane(src, W, H)
                peak = max(peak, top)
                assert int(np.abs(got.astype(np.int64) - R.resize_real(src, W, H)).max()) <= 1, (sw, sh, W, H)
                if (W, H) == (sw, sh):
                    assert np.array_equal(got, src)
                if (2 * W, 2 * H) == (sw, sh):
                    s = src.astype(np.int64)
                    assert np.array_equal(got, (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2)
    assert peak < 1 << 24


def test_the_float_step_is_two_roundings():
    c = np.arange(256, dtype=np.uint8)
    s, b = 1 / (255 * 0.229), -0.485 / 0.229
    f = R.to_float(c, s, b, "f32")
    assert f.dtype == np.float32 and np.array_equal(f, (c.astype(np.float32) * np.float32(s)) + np.float32(b))
    assert np.array_equal(R.to_float(c, s, b, "f16"), f.astype(np.float16))
    fused = (c.astype(np.float64) * np.float64(np.float32(s)) + np.float64(np.float32(b))).astype(np.float32)
    assert np.any(fused != f)                                # (a fused multiply-add would differ: the checker can tell)


@pytest.mark.parametrize("fmt", X.FORMATS)
def test_frame_bytes_is_the_layout_table(lib, fmt):
    for dtype, elem in (("u8", 1), ("f16", 2), ("f32", 4)):
        if dtype != "u8" and not fmt.startswith("rgb"):
            continue
        for W, H in ((80, 48), (34, 18), (2, 2), (224, 224), (16384, 16384)):
            tight = (3 * W if fmt == "rgb24" else W) * elem
            for pitch in (0, tight, tight + 16, tight + 2 * elem):
                p = pitch or tight
                want = {"i420": p * H * 3 // 2, "nv12": p * H * 3 // 2, "rgb24": p * H, "rgbp": 3 * p * H}[fmt]
                r = desc(fmt, (W, H), (0, 0, 1920, 1080), dtype=dtype, pitch=pitch)
                assert lib.p264hip_resize_frame_bytes(C.byref(r)) == want == R.frame_bytes(fmt, W, H, dtype, pitch)
                assert lib.p264hip_resize_check(C.byref(r), 120, 68) == 0
                for stride, ok in ((want, True), (want + 8, True), (want - elem, False)):
                    r.frame_stride = stride
                    assert (lib.p264hip_resize_check(C.byref(r), 120, 68) == 0) == ok


def test_the_refusals(lib):
    fb, chk = lib.p264hip_resize_frame_bytes, lambda r: lib.p264hip_resize_check(C.byref(r), 5, 3)
    assert fb(None) == EINVAL and lib.p264hip_resize_check(None, 5, 3) == EINVAL
    inf, nan = float("inf"), float("nan")
    # (refused, the accepted case beside it)
    pairs = [
        # what p264hip_export_check refuses for the fields the two share
        (desc(fmt=4), desc(fmt=3)), (desc(fmt=-1), desc(fmt=0)), (desc("rgb24", matrix=2), desc("rgb24", matrix=1)), (desc("rgbp", matrix=-1), desc("rgbp", matrix=0)),
        (desc("i420", matrix="bt709"), desc("i420")), (desc("nv12", full_range=True), desc("nv12")), (desc("rgb24", full_range=2), desc("rgb24", full_range=1)),
        (desc(crop=(1, 0, 62, 30)), desc(crop=(2, 0, 62, 30))), (desc(crop=(0, 1, 62, 30)), desc(crop=(0, 2, 62, 30))),
        (desc(crop=(0, 0, 61, 30)), desc(crop=(0, 0, 62, 30))), (desc(crop=(0, 0, 62, 29)), desc(crop=(0, 0, 62, 30))),
        (desc(crop=(0, 0, 0, 30)), desc(crop=(0, 0, 2, 30))), (desc(crop=(0, 0, 62, 0)), desc(crop=(0, 0, 62, 2))),
        (desc(crop=(-2, 0, 62, 30)), desc(crop=(0, 0, 62, 30))), (desc(crop=(0, -2, 62, 30)), desc(crop=(0, 0, 62, 30))),
        (desc("i420", pitch=35), desc("i420", pitch=36)), (desc("rgbp", pitch=-34), desc("rgbp", pitch=35)),
        # an unknown dtype or filter; a float dtype on a YUV format
        (desc(dtype=3), desc(dtype=2)), (desc(dtype=-1), desc(dtype=0)), (desc(filter=1), desc(filter=0)), (desc(filter=-1), desc(filter=0)),
        (desc("i420", dtype="f16"), desc("rgbp", dtype="f16")), (desc("nv12", dtype="f32"), desc("rgb24", dtype="f32")),
        # scale / bias: not 0 where the dtype is U8, not finite anywhere
        (desc(scale=1 / 255), desc(dtype="f32", scale=1 / 255)), (desc(bias=(0, 0, 1)), desc(dtype="f16", bias=(0, 0, 1))),
        (desc(scale=(0, nan, 0)), desc(scale=(0, 0, 0))), (desc(bias=(inf, 0, 0)), desc(bias=None)),
        (desc(dtype="f32", scale=(1, inf, 1)), desc(dtype="f32", scale=(1, 3e38, 1))), (desc(dtype="f16", bias=(0, 0, nan)), desc(dtype="f16", bias=(0, 0, -2))),
        (desc(dtype="f32", scale=-inf), desc(dtype="f32", scale=-1)),
        # a pitch below the tight one, or no multiple of the element size
        (desc(pitch=32), desc(pitch=34)), (desc("rgb24", pitch=100), desc("rgb24", pitch=102)),
        (desc(dtype="f16", pitch=66), desc(dtype="f16", pitch=68)), (desc(dtype="f16", pitch=71), desc(dtype="f16", pitch=72)),
        (desc(dtype="f32", pitch=138), desc(dtype="f32", pitch=140)), (desc("rgb24", dtype="f32", pitch=404), desc("rgb24", dtype="f32", pitch=408)),
        # an output size that is odd, below 2 or above 16384
        (desc(size=(33, 18)), desc(size=(32, 18))), (desc(size=(34, 17)), desc(size=(34, 16))), (desc(size=(0, 18)), desc(size=(2, 18))),
        (desc(size=(34, 0)), desc(size=(34, 2))), (desc(size=(-2, 18)), desc(size=(2, 18))), (desc(size=(16386, 18)), desc(size=(16384, 18))),
        (desc(size=(34, 16386)), desc(size=(34, 16384))),
    ]
    for i, (bad, good) in enumerate(pairs):
        assert fb(C.byref(bad)) == EINVAL and chk(bad) == EINVAL, i
        assert fb(C.byref(good)) > 0 and chk(good) == 0, i
    # the frame: 5 x 3 macroblocks = 80 x 48
    for crop in ((0, 0, 82, 48), (0, 0, 80, 50), (2, 0, 80, 48), (0, 2, 80, 48), (80, 0, 2, 2), (0, 48, 2, 2)):
        r = desc(crop=crop)
        assert fb(C.byref(r)) > 0 and chk(r) == EINVAL, crop
    assert chk(desc(crop=(78, 46, 2, 2))) == 0
    for mb in ((0, 3), (5, 0), (-1, 3)):
        assert lib.p264hip_resize_check(C.byref(desc(crop=(0, 0, 2, 2))), *mb) == EINVAL
    # a frame_stride below the picture's bytes (or no multiple of the element size)
    per = 3 * 34 * 18
    for r, stride, ok in ((desc(), per - 1, False), (desc(), per, True), (desc(), -8, False), (desc(dtype="f16"), 2 * per - 2, False), (desc(dtype="f16"), 2 * per + 2, True),
                          (desc(dtype="f16"), 2 * per + 1, False), (desc(dtype="f32"), 4 * per + 6, False), (desc(dtype="f32"), 4 * per + 8, True)):
        r.frame_stride = stride
        assert fb(C.byref(r)) > 0 and (chk(r) == 0) == ok, (r.dtype, stride)


def test_abi_mirror(lib):
    import os
    import subprocess
    import tempfile
    names = [n for n, _ in N.Resize._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "p264pipe.h"\nint main(void) { printf("%zu %zu", sizeof(p264hip_resize_t), sizeof(p264hip_export_t));\n'
           + "".join('printf(" %%zu", offsetof(p264hip_resize_t, %s));\n' % n for n in names) + 'printf("\\n"); return 0; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I" + inc, os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(td, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(N.Resize) == 80 and out[1] == 40
    assert out[2:] == [getattr(N.Resize, n).offset for n in names]
    assert (N.DTYPE_U8, N.DTYPE_F16, N.DTYPE_F32, N.FILTER_BILINEAR) == (0, 1, 2, 0)
    for f in ("p264hip_resize_frame_bytes", "p264hip_resize_check", "p264hip_resize_taps", "p264hip_export_resized"):
        assert hasattr(lib, f)
    # format 4 of the plain export stays refused
    assert lib.p264hip_export_check(C.byref(N.export_desc(4, (0, 0, 80, 48), None)), 5, 3) == EINVAL


def test_the_kernels_are_in_the_code_object_without_spills_scratch_or_lds(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for k in KERNELS:
        assert k in res, sorted(res)
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
