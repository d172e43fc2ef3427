"""The host side of the antialiased filter of the resized device export (include/p264hip.h: P264HIP_FILTER_BILINEAR_AA), no GPU: the
taps of p264hip_resize_aa_taps against the numpy model of tests/resize_aa_checker.py and against the definition in exact fractions,
the model against the real-valued filter (inside the derived bound) and against torch's antialiased interpolate on the CPU, the
descriptions p264hip_resize_frame_bytes / p264hip_resize_check accept and refuse with filter = 2, the Python names, and the kernels
in the code object."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests.test_resize_cpu import desc as desc0

EINVAL = -1
PAIRS = [(2, 2), (2, 16384), (80, 80), (80, 40), (80, 34), (48, 98), (40, 2), (1080, 224), (1920, 640), (1920, 60), (64, 2)]
KERNELS = ("k_resize_aa_i420", "k_resize_aa_nv12", "k_resize_aa_rgb24_u8", "k_resize_aa_rgb24_f16", "k_resize_aa_rgb24_f32",
           "k_resize_aa_rgbp_u8", "k_resize_aa_rgbp_f16", "k_resize_aa_rgbp_f32")
PLANES = [(80, 48), (62, 30), (2, 2), (304, 144)]           # (width, height)
SIZES = [None, "half", (34, 18), (162, 98), (4, 2), (6, 70), (224, 224), (10, 6)]


def desc(*a, **kw):
    kw.setdefault("filter", "bilinear_aa")
    return desc0(*a, **kw)


def host_taps(lib, S, D):
    first, count, w = (C.c_int32 * D)(), (C.c_int32 * D)(), (C.c_uint16 * (D * 64))()
    assert lib.p264hip_resize_aa_taps(S, D, first, count, w) == 0
    return np.ctypeslib.as_array(first).astype(np.int64), np.ctypeslib.as_array(count).astype(np.int64), np.ctypeslib.as_array(w).astype(np.int64).reshape(D, 64)


@pytest.mark.parametrize("S,D", PAIRS)
def test_host_taps_are_the_model(lib, S, D):
    first, count, w = host_taps(lib, S, D)
    mf, mc, mw = A.aa_taps(S, D)
    assert np.array_equal(first, mf) and np.array_equal(count, mc) and np.array_equal(w, mw)
    assert np.all(w.sum(axis=1) == 32768) and count.min() >= 1 and count.max() <= 64
    assert first.min() >= 0 and np.all(first + count <= S)
    assert np.all(w[np.arange(64)[None, :] >= count[:, None]] == 0) and np.all(w[np.arange(64)[None, :] < count[:, None]] >= 0)


@pytest.mark.parametrize("S,D", PAIRS)
def test_host_taps_are_the_definition_in_exact_fractions(lib, S, D):
    first, count, w = host_taps(lib, S, D)
    U = 2 * max(S, D)
    step = max(1, D // 499)                                  # (every index of the short axes, five hundred of the long one, both ends)
    for d in sorted((set(range(0, D, step)) | {0, 1, D - 2, D - 1}) & set(range(D))):
        # the triangle over EVERY source index, straight from the definition: centre and half-width in source samples
        centre, half = Fraction(2 * d + 1, 2) * Fraction(S, D), Fraction(U, 2 * D)
        r = [max(Fraction(0), 1 - abs(Fraction(2 * j + 1, 2) - centre) / half) for j in range(S)] if S <= 128 else None
        if r is None:                                       # (a long axis: the indices around the centre, two samples beyond the support)
            lo, hi = max(int(centre - half) - 2, 0), min(int(centre + half) + 2, S - 1)
            r = [Fraction(0)] * lo + [max(Fraction(0), 1 - abs(Fraction(2 * j + 1, 2) - centre) / half) for j in range(lo, hi + 1)]
        taps = [j for j, x in enumerate(r) if x > 0]
        assert taps == list(range(first[d], first[d] + count[d])), (S, D, d)
        total = sum(r)
        want = [int(r[j] * 32768 / total) for j in taps]
        want[max(range(len(taps)), key=lambda k: (r[taps[k]], -k))] += 32768 - sum(want)
        assert want == list(w[d, :count[d]]), (S, D, d)


def test_taps_refusals(lib):
    f, c, w = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_uint16 * 256)()
    assert lib.p264hip_resize_aa_taps(2, 4, f, c, w) == 0 and lib.p264hip_resize_aa_taps(128, 4, f, c, w) == 0
    for S, D, a in ((2, 4, (None, c, w)), (2, 4, (f, None, w)), (2, 4, (f, c, None)), (0, 4, (f, c, w)), (-1, 4, (f, c, w)), (2, 0, (f, c, w)), (2, -1, (f, c, w)),
                    ((1 << 20) + 1, 1 << 20, (None, None, None)), (2, (1 << 20) + 1, (None, None, None)), (129, 4, (f, c, w))):
        assert lib.p264hip_resize_aa_taps(S, D, *a) == EINVAL, (S, D)
    big = 1 << 20
    f, c, w = (C.c_int32 * 1)(), (C.c_int32 * 1)(), (C.c_uint16 * 64)()
    assert lib.p264hip_resize_aa_taps(big + 1, big, f, c, w) == EINVAL and lib.p264hip_resize_aa_taps(33, 1, f, c, w) == EINVAL      # 2^20 + 1; S = 32 D + 1
    assert lib.p264hip_resize_aa_taps(32, 1, f, c, w) == 0 and c[0] == 32


def sources(g, sw, sh):
    yy, xx = np.mgrid[0:sh, 0:sw]
    return (g.integers(0, 256, (sh, sw), np.uint8), (((xx + yy) & 1) * 255).astype(np.uint8), np.full((sh, sw), 255, np.uint8))


def plane_cases():
    """(source, W, H) of the two model tests: random, checkerboard and constant-255 planes at every size the limit allows"""
    g = np.random.default_rng(2660)
    for sw, sh in PLANES:
        srcs = sources(g, sw, sh)
        for size in SIZES:
            W, H = (sw, sh) if size is None else (sw // 2, sh // 2) if size == "half" else size
            if W < 1 or H < 1 or sw > 32 * W or sh > 32 * H:
                continue
            for src in srcs:
                yield src, W, H


def test_the_model_is_within_the_derived_bound_of_the_real_filter():
    top1 = top2 = n = 0
    worst = 0.0
    for src, W, H in plane_cases():
        sh, sw = src.shape
        got, s1, s2, (nx, ny) = A.resize_plane_aa(src, W, H)
        top1, top2, n = max(top1, s1), max(top2, s2), n + 1
        err = float(np.abs(got.astype(np.float64) - A.real_aa(src, W, H)).max())
        worst = max(worst, err)
        assert err <= A.bound(nx, ny), (sw, sh, W, H, err, A.bound(nx, ny))
        if (W, H) == (sw, sh):
            assert np.array_equal(got, src)
        if np.all(src == 255):
            assert np.all(got == 255)
    assert n >= 60 and top1 < 1 << 23 and top2 < 1 << 30, (n, top1, top2)
    # D == S / 2: the interior weights are 1, 3, 3, 1 over 8
    first, count, w = A.aa_taps(80, 40)
    assert np.all(count[1:-1] == 4) and np.all(w[1:-1, :4] == [4096, 12288, 12288, 4096]) and np.array_equal(first[1:-1], 2 * np.arange(1, 39) - 1)
    assert list(w[0, :3]) == [3 * 32768 // 7 + 1, 3 * 32768 // 7, 32768 // 7] and count[0] == 3         # (the edge: 3, 3, 1 over 7, the rest to the first of the equals)


def test_the_model_against_torch_on_the_cpu():
    torch = pytest.importorskip("torch")
    F = torch.nn.functional
    try:
        F.interpolate(torch.zeros(1, 1, 4, 4), size=(2, 2), mode="bilinear", align_corners=False, antialias=True)
    except (TypeError, RuntimeError, NotImplementedError) as e:
        pytest.skip("this torch has no antialiased interpolate: %s" % e)
    worst = 0.0
    for src, W, H in plane_cases():
        got, _, _, (nx, ny) = A.resize_plane_aa(src, W, H)
        ref = F.interpolate(torch.from_numpy(src.astype(np.float32))[None, None], size=(H, W), mode="bilinear", align_corners=False, antialias=True)[0, 0].numpy()
        err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        worst = max(worst, err)
        # (the issue's bound: 1/2 + the derived bound + 0.01 for torch's own float32 weights)
        assert err <= 0.5 + A.bound(nx, ny) + 0.01, "%s to %dx%d: %.4f from torch (largest so far %.4f)" % (src.shape, W, H, err, worst)
    print("largest difference from torch: %.4f" % worst)


def test_descriptions_with_the_antialiased_filter(lib):
    fb, chk = lib.p264hip_resize_frame_bytes, lambda r: lib.p264hip_resize_check(C.byref(r), 5, 3)
    for fmt, dtype in (("i420", "u8"), ("nv12", "u8"), ("rgb24", "u8"), ("rgbp", "u8"), ("rgb24", "f16"), ("rgbp", "f32")):
        for size in ((80, 48), (34, 18), (162, 98), (4, 2), (16384, 16384)):
            for pitch in (0, R.tight_pitch(fmt, size[0], dtype) + 16):
                a, b = desc0(fmt, size, dtype=dtype, pitch=pitch), desc(fmt, size, dtype=dtype, pitch=pitch)
                assert b.filter == 2 and fb(C.byref(a)) == fb(C.byref(b)) == R.frame_bytes(fmt, size[0], size[1], dtype, pitch) and chk(a) == chk(b) == 0
    # the limit: a window more than 32 times the output, in either direction; filter 0 has no such limit
    for size, crop, ok in (((2, 2), (0, 0, 80, 48), False), ((4, 2), (0, 0, 80, 48), True), ((2, 2), (0, 0, 64, 48), True), ((2, 2), (0, 0, 66, 48), False),
                           ((80, 2), (0, 0, 80, 64), True), ((80, 2), (0, 0, 80, 66), False)):
        r = desc(size=size, crop=crop)
        assert (fb(C.byref(r)) > 0) == ok and (lib.p264hip_resize_check(C.byref(r), 5, 5) == 0) == ok, (size, crop)
        assert fb(C.byref(desc0(size=size, crop=crop))) > 0


def test_the_refusals_hold_with_the_antialiased_filter(lib):
    """the pairs of tests/test_resize_cpu.py::test_the_refusals with filter = 2 in every description: what was refused is refused, what
    was accepted is accepted.  Two of its accepted cases, a width of 2 from the 80 columns of the default window, are above 32:1; they
    take a window of 62 x 30 here.  The two filter pairs set the filter against 2."""
    fb, chk = lib.p264hip_resize_frame_bytes, lambda r: lib.p264hip_resize_check(C.byref(r), 5, 3)
    inf, nan = float("inf"), float("nan")
    narrow = (0, 0, 62, 30)
    pairs = [
        (desc(fmt=4), desc(fmt=3)), (desc(fmt=-1), desc(fmt=0)), (desc("rgb24", matrix=2), desc("rgb24", matrix=1)), (desc("rgbp", matrix=-1), desc("rgbp", matrix=0)),
        (desc("i420", matrix="bt709"), desc("i420")), (desc("nv12", full_range=True), desc("nv12")), (desc("rgb24", full_range=2), desc("rgb24", full_range=1)),
        (desc(crop=(1, 0, 62, 30)), desc(crop=(2, 0, 62, 30))), (desc(crop=(0, 1, 62, 30)), desc(crop=(0, 2, 62, 30))),
        (desc(crop=(0, 0, 61, 30)), desc(crop=(0, 0, 62, 30))), (desc(crop=(0, 0, 62, 29)), desc(crop=(0, 0, 62, 30))),
        (desc(crop=(0, 0, 0, 30)), desc(crop=(0, 0, 2, 30))), (desc(crop=(0, 0, 62, 0)), desc(crop=(0, 0, 62, 2))),
        (desc(crop=(-2, 0, 62, 30)), desc(crop=(0, 0, 62, 30))), (desc(crop=(0, -2, 62, 30)), desc(crop=(0, 0, 62, 30))),
        (desc("i420", pitch=35), desc("i420", pitch=36)), (desc("rgbp", pitch=-34), desc("rgbp", pitch=35)),
        (desc(dtype=3), desc(dtype=2)), (desc(dtype=-1), desc(dtype=0)), (desc(filter=1), desc(filter=2)), (desc(filter=-1), desc(filter=2)),
        (desc(filter=3), desc(filter=0)),
        (desc("i420", dtype="f16"), desc("rgbp", dtype="f16")), (desc("nv12", dtype="f32"), desc("rgb24", dtype="f32")),
        (desc(scale=1 / 255), desc(dtype="f32", scale=1 / 255)), (desc(bias=(0, 0, 1)), desc(dtype="f16", bias=(0, 0, 1))),
        (desc(scale=(0, nan, 0)), desc(scale=(0, 0, 0))), (desc(bias=(inf, 0, 0)), desc(bias=None)),
        (desc(dtype="f32", scale=(1, inf, 1)), desc(dtype="f32", scale=(1, 3e38, 1))), (desc(dtype="f16", bias=(0, 0, nan)), desc(dtype="f16", bias=(0, 0, -2))),
        (desc(dtype="f32", scale=-inf), desc(dtype="f32", scale=-1)),
        (desc(pitch=32), desc(pitch=34)), (desc("rgb24", pitch=100), desc("rgb24", pitch=102)),
        (desc(dtype="f16", pitch=66), desc(dtype="f16", pitch=68)), (desc(dtype="f16", pitch=71), desc(dtype="f16", pitch=72)),
        (desc(dtype="f32", pitch=138), desc(dtype="f32", pitch=140)), (desc("rgb24", dtype="f32", pitch=404), desc("rgb24", dtype="f32", pitch=408)),
        (desc(size=(33, 18)), desc(size=(32, 18))), (desc(size=(34, 17)), desc(size=(34, 16))), (desc(size=(0, 18), crop=narrow), desc(size=(2, 18), crop=narrow)),
        (desc(size=(34, 0)), desc(size=(34, 2))), (desc(size=(-2, 18), crop=narrow), desc(size=(2, 18), crop=narrow)), (desc(size=(16386, 18)), desc(size=(16384, 18))),
        (desc(size=(34, 16386)), desc(size=(34, 16384))),
    ]
    assert len(pairs) == 44
    for i, (bad, good) in enumerate(pairs):
        assert fb(C.byref(bad)) == EINVAL and chk(bad) == EINVAL, i
        assert fb(C.byref(good)) > 0 and chk(good) == 0, i
    for crop in ((0, 0, 82, 48), (0, 0, 80, 50), (2, 0, 80, 48), (0, 2, 80, 48), (80, 0, 2, 2), (0, 48, 2, 2)):
        r = desc(crop=crop)
        assert fb(C.byref(r)) > 0 and chk(r) == EINVAL, crop
    assert chk(desc(crop=(78, 46, 2, 2))) == 0
    per = 3 * 34 * 18
    for r, stride, ok in ((desc(), per - 1, False), (desc(), per, True), (desc(), -8, False), (desc(dtype="f16"), 2 * per - 2, False), (desc(dtype="f16"), 2 * per + 2, True),
                          (desc(dtype="f16"), 2 * per + 1, False), (desc(dtype="f32"), 4 * per + 6, False), (desc(dtype="f32"), 4 * per + 8, True)):
        r.frame_stride = stride
        assert fb(C.byref(r)) > 0 and (chk(r) == 0) == ok, (r.dtype, stride)


def test_python_names(lib):
    assert N.FILTER_BILINEAR == 0 and N.FILTER_BILINEAR_AA == 2
    frame = (80, 48)
    assert N.resize_desc(frame=frame, filter="bilinear_aa").filter == 2 and N.resize_desc(frame=frame, filter="bilinear").filter == 0 and N.resize_desc(frame=frame).filter == 0
    assert N.resize_desc(frame=frame, filter=2).filter == 2 and N.resize_desc(frame=frame, filter=1).filter == 1
    with pytest.raises(KeyError):
        N.resize_desc(frame=frame, filter="box")
    assert C.sizeof(N.Resize) == 80 and hasattr(lib, "p264hip_resize_aa_taps")
    import inspect
    from p264decoder_amd import HipReconstructor, Pipeline
    for f in (HipReconstructor.export_resized, Pipeline.export_last_resized, Pipeline.set_sink_resized):
        p = inspect.signature(f).parameters["filter"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "bilinear"


def test_the_kernels_are_in_the_code_object_without_spills_or_scratch(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for k in KERNELS:
        assert k in res, sorted(res)
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] <= 65536, (k, r)
