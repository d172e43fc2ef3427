"""The host side of the export of per-picture windows with the antialiased filter (include/p264hip.h: p264hip_export_rois_aa), no GPU:
the refusals of p264hip_rois_aa_check / p264hip_rois_aa_frame_bytes, the two closed-form bounds a segment and a tile are sized by, the
segment p264hip_roi_aa_segment writes - the text k_roi_aa_taps runs - word for word against tests/resize_aa_checker.aa_taps, the numpy
model of tests/roi_aa_checker.py against the models it is built on, and the nine kernels in the code object."""
import ctypes as C
import inspect

import numpy as np
import pytest

import p264decoder_amd
from p264decoder_amd import _native as N
from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K
from tests import test_roi_cpu as T0

EINVAL = -1
MB_W, MB_H, STREAMS, SLOTS = T0.MB_W, T0.MB_H, T0.STREAMS, T0.SLOTS
INSTANCES = T0.INSTANCES
KERNELS = ("k_roi_aa_taps",) + tuple("k_roi_aa_" + k[len("k_roi_"):] for k in T0.KERNELS[1:])
FILL_WORD = T0.FILL_WORD
AA = N.FILTER_BILINEAR_AA
T_CAP = 20480                                               # P264HIP_ROI_AA_TILE_VALUES


def desc(fmt="rgbp", size=(34, 18), crop=(0, 0, 2, 2), filter=AA, **kw):
    return N.resize_desc(fmt, size, crop, None, filter=filter, **kw)


roi = T0.roi


def check(lib, rois, r, fill=FILL_WORD, n=None, mb=(MB_W, MB_H), store=(STREAMS, SLOTS)):
    arr = (N.Roi * len(rois))(*rois) if rois is not None else None
    return lib.p264hip_rois_aa_check(arr, len(rois) if n is None else n, C.byref(r) if r is not None else None, fill, mb[0], mb[1], store[0], store[1])


def test_the_filter_must_be_the_antialiased_one(lib):
    one = [roi()]
    assert check(lib, one, desc()) == 0 and lib.p264hip_rois_aa_frame_bytes(C.byref(desc())) == 3 * 34 * 18
    for f in (0, 1, -1):
        assert check(lib, one, desc(filter=f)) == EINVAL, f
        assert lib.p264hip_rois_aa_frame_bytes(C.byref(desc(filter=f))) == EINVAL, f
    assert lib.p264hip_rois_aa_frame_bytes(None) == EINVAL
    # ... and the filter-0 entry points refuse it still
    assert lib.p264hip_rois_check((N.Roi * 1)(*one), 1, C.byref(desc()), FILL_WORD, MB_W, MB_H, STREAMS, SLOTS) == EINVAL
    assert lib.p264hip_rois_frame_bytes(C.byref(desc())) == EINVAL


def test_the_refusals_of_the_description_with_filter_2(lib):
    """the pairs of tests/test_roi_cpu.py's description table (refused, accepted), with filter 2 set, through the new entry points"""
    fb = lib.p264hip_rois_aa_frame_bytes
    inf, nan = float("inf"), float("nan")
    pairs = [
        # format, matrix, range
        (desc(fmt=4), desc(fmt=3)), (desc(fmt=-1), desc(fmt=0)), (desc("rgb24", matrix=2), desc("rgb24", matrix=1)),
        (desc("i420", matrix="bt709"), desc("i420")), (desc("nv12", full_range=True), desc("nv12")), (desc("rgb24", full_range=2), desc("rgb24", full_range=1)),
        # dtype
        (desc(dtype=3), desc(dtype=2)), (desc(dtype=-1), desc(dtype=0)), (desc("i420", dtype="f16"), desc("rgbp", dtype="f16")), (desc("nv12", dtype="f32"), desc("rgb24", dtype="f32")),
        # scale / bias
        (desc(scale=1 / 255), desc(dtype="f32", scale=1 / 255)), (desc(bias=(0, 0, 1)), desc(dtype="f16", bias=(0, 0, 1))),
        (desc(scale=(0, nan, 0)), desc(scale=(0, 0, 0))), (desc(dtype="f32", scale=(1, inf, 1)), desc(dtype="f32", scale=(1, 3e38, 1))),
        # pitch
        (desc(pitch=32), desc(pitch=34)), (desc("i420", pitch=35), desc("i420", pitch=36)), (desc("rgb24", pitch=100), desc("rgb24", pitch=102)),
        (desc(dtype="f16", pitch=71), desc(dtype="f16", pitch=72)), (desc(dtype="f32", pitch=138), desc(dtype="f32", pitch=140)),
        # the output size
        (desc(size=(33, 18)), desc(size=(34, 18))), (desc(size=(34, 17)), desc(size=(34, 18))), (desc(size=(0, 18)), desc(size=(2, 18))),
        (desc(size=(16386, 18)), desc(size=(16384, 18))), (desc(size=(34, 16386)), desc(size=(34, 16384))),
    ]
    one = [roi(window=(0, 0, 2, 2), rect=(0, 0, 2, 2))]
    for i, (bad, good) in enumerate(pairs):
        assert bad.filter == good.filter == AA
        assert fb(C.byref(bad)) == EINVAL and check(lib, one, bad) == EINVAL, i
        assert fb(C.byref(good)) > 0 and check(lib, one, good) == 0, i
    # a frame_stride below the picture's bytes, or no multiple of the element size
    per = 3 * 34 * 18
    for r, stride, ok in ((desc(), per - 1, False), (desc(), per, True), (desc(), -8, False), (desc(dtype="f16"), 2 * per + 2, True), (desc(dtype="f16"), 2 * per + 1, False),
                          (desc(dtype="f32"), 4 * per + 6, False), (desc(dtype="f32"), 4 * per + 8, True)):
        r.frame_stride = stride
        assert fb(C.byref(r)) > 0 and (check(lib, one, r) == 0) == ok, (r.dtype, stride)


def test_the_refusals_of_the_roi_list_hold(lib):
    """what p264hip_rois_check refuses in a list, p264hip_rois_aa_check refuses: a sample of each kind, in any place of the list"""
    good = roi()
    for bad in (roi(window=(1, 2, 62, 30)), roi(window=(2, 2, 0, 30)), roi(window=(20, 0, 62, 30)), roi(window=(0, 0, 80, 50)), roi(rect=(1, 2, 30, 14)),
                roi(rect=(6, 0, 30, 18)), roi(rect=(0, 0, 34, 0)), roi(rect=(0, 18, 2, 2)), roi(stream=STREAMS), roi(slot=-1)):
        assert check(lib, [bad], desc()) == EINVAL
        assert check(lib, [good, good, bad], desc()) == EINVAL and check(lib, [bad, good], desc()) == EINVAL
    assert check(lib, [good], desc(), n=0) == EINVAL and check(lib, [good], None) == EINVAL
    assert lib.p264hip_rois_aa_check(None, 1, C.byref(desc()), FILL_WORD, MB_W, MB_H, STREAMS, SLOTS) == EINVAL
    assert check(lib, [good], desc(), fill=1 << 24) == EINVAL and check(lib, [good], desc(), fill=0xffffff) == 0
    assert check(lib, [good], desc(), mb=(0, 3)) == EINVAL and check(lib, [good], desc(), store=(0, 2)) == EINVAL
    assert check(lib, [roi(2, 1, (0, 0, 80, 48)), roi(0, 0, (78, 46, 2, 2), (32, 16, 2, 2))], desc()) == 0


def test_the_limit_of_32_to_1_is_per_roi(lib):
    big = (8, 8)                                            # a 128 x 128 frame
    r = desc(size=(34, 18))
    good = roi(window=(0, 0, 62, 30))
    # at its edge, in width and in height: 64 into 2 is accepted, 66 is not
    for ok, o in ((True, roi(window=(0, 0, 64, 2), rect=(4, 4, 2, 2))), (False, roi(window=(0, 0, 66, 2), rect=(4, 4, 2, 2))),
                  (True, roi(window=(0, 0, 2, 64), rect=(4, 4, 2, 2))), (False, roi(window=(0, 0, 2, 66), rect=(4, 4, 2, 2))),
                  (True, roi(window=(62, 62, 64, 64), rect=(32, 16, 2, 2))), (True, roi(window=(0, 0, 128, 128), rect=(0, 0, 4, 4))),
                  (False, roi(window=(0, 0, 128, 128), rect=(0, 0, 4, 2))), (False, roi(window=(0, 0, 128, 128), rect=(0, 0, 2, 4)))):
        assert (check(lib, [o], r, mb=big) == 0) == ok, bytes(o)
        for rois in ([o, good, good], [good, o, good], [good, good, o]):    # the bad ROI in any place of the list
            assert (check(lib, rois, r, mb=big) == 0) == ok
    # the whole output where the rectangle is all 0: 2 x 2 takes 64 x 64 and no more
    small = desc(size=(2, 2))
    assert check(lib, [roi(window=(0, 0, 64, 64))], small, mb=big) == 0
    assert check(lib, [roi(window=(0, 0, 66, 64))], small, mb=big) == EINVAL and check(lib, [roi(window=(0, 0, 64, 66))], small, mb=big) == EINVAL
    assert check(lib, [roi(window=(0, 0, 66, 64), rect=(0, 0, 2, 2))], small, mb=big) == EINVAL
    # the description's own crop_* are not read: a window p264hip_resize_check would refuse for its ratio changes nothing
    assert check(lib, [good], desc(crop=(0, 0, 1920, 1080), size=(2, 2))) == 0
    # the filter-0 call has no such limit
    assert lib.p264hip_rois_check((N.Roi * 1)(roi(window=(0, 0, 128, 128), rect=(0, 0, 2, 2))), 1, C.byref(desc(filter=0)), FILL_WORD, 8, 8, STREAMS, SLOTS) == 0


# ---- the two bounds
def sweep():
    """(S, D) pairs: every S, D up to 40 within 32:1, and seeded pairs up to 1100 x 256; the named pairs first"""
    pairs = [(1920, 60), (1080, 34), (64, 2), (960, 30), (540, 17), (32, 1), (1920, 224), (1080, 126), (1916, 224), (200, 224)]
    pairs += [(s, d) for s in range(1, 41) for d in range(1, 41) if s <= 32 * d]
    g = np.random.default_rng(2671)
    while len(pairs) < 8716:
        s, d = int(g.integers(1, 1101)), int(g.integers(1, 257))
        if s <= 32 * d:
            pairs.append((s, d))
    return pairs


def test_the_stride_bound_and_the_span_bound():
    """no count exceeds the stride, and a tile of tw destination samples spans no more source samples than the closed form says -
    from every start, even or odd, not only multiples of the tile"""
    n = 0
    for S, D in sweep():
        first, count, _ = KA.taps(S, D)
        st = KA.stride(S, D)
        assert count.max() <= st <= 64 and st % 2 == 0, (S, D, int(count.max()), st)
        last = first + count - 1
        for tw in (64, 32, 16, 8, 4):
            tw_eff = min(tw, D)
            x0 = np.arange(0, D - tw_eff + 1)
            span = last[x0 + tw_eff - 1] - first[x0] + 1
            assert span.max() <= min(KA.span_bound(S, D, tw_eff), S) <= KA.span_bound(S, D, tw), (S, D, tw, int(span.max()))
        n += 1
    assert n >= 8716


def test_the_tile_width_the_host_chooses(lib):
    """p264hip_roi_aa_tile_width: the widest tile whose closed-form span fits the LDS, per ROI - and the real span fits its strips"""
    r = desc(size=(224, 224))
    for window, rect, tw in (((0, 0, 1920, 1080), (0, 0, 0, 0), 64), ((0, 0, 1920, 1080), (82, 94, 60, 34), 32), ((0, 0, 64, 32), (0, 0, 2, 2), 64),
                             ((0, 0, 640, 640), (0, 0, 0, 0), 64), ((0, 0, 62, 30), (0, 0, 0, 0), 64), ((0, 0, 1920, 1080), (0, 0, 64, 34), 32)):
        o = roi(window=window, rect=rect)
        nl, nc = C.c_int(), C.c_int()
        got = lib.p264hip_roi_aa_tile_width(C.byref(o), C.byref(r), C.byref(nl), C.byref(nc))
        S, D = window[2], rect[2] or 224
        assert got in (64, 32, 16, 8) and nl.value * 256 <= T_CAP and nc.value * 128 <= T_CAP, (window, rect, got)
        # the widest of 64, 32, 16, 8 whose span - the closed form, and no more than the window - fits T_CAP values in both planes
        fits = [t for t in (64, 32, 16, 8) if (min(KA.span_bound(S, D, t), S) + 30) // 16 * 256 <= T_CAP and (min(KA.span_bound(S // 2, D // 2, t // 2), S // 2) + 14) // 8 * 128 <= T_CAP]
        assert got == fits[0] == tw, (window, rect, got, fits)
        # the strips of any tile of the axis, at the window's offset in the frame, fit
        for left in (0, 2, 14):
            for (s, d, sh, strips, t) in ((S, D, 4, nl.value, got), (S // 2, D // 2, 3, nc.value, got // 2)):
                first, count, _ = KA.taps(s, d)
                off = left >> (4 - sh)
                for x0 in range(0, d, 1):
                    x1 = min(x0 + t, d) - 1
                    assert ((off + first[x1] + count[x1] - 1) >> sh) - ((off + first[x0]) >> sh) + 1 <= strips, (window, rect, left, x0)
    assert lib.p264hip_roi_aa_tile_width(C.byref(roi(window=(0, 0, 66, 2), rect=(0, 0, 2, 2))), C.byref(r), None, None) == EINVAL


# ---- the segment
SEGMENTS = [
    # window (it begins inside a strip), rectangle size: S < D, S == D, 2:1, an odd ratio, 32:1 / 16:1, and mixtures
    ((18, 6, 30, 14), (62, 34)), ((18, 6, 30, 14), (30, 14)), ((18, 6, 60, 28), (30, 14)), ((6, 2, 70, 46), (22, 10)), ((2, 4, 64, 32), (2, 2)),
    ((10, 2, 64, 14), (2, 30)), ((4, 4, 62, 30), (34, 18)), ((0, 0, 80, 48), (162, 98)), ((2, 2, 2, 2), (2, 2)), ((34, 18, 46, 30), (6, 70)),
    ((2, 4, 1916, 1072), (224, 126)), ((0, 0, 1920, 1080), (60, 34)),
]


@pytest.mark.parametrize("window,rect_size", SEGMENTS)
def test_the_segment_word_for_word(lib, window, rect_size):
    r = desc(size=(518, 256))
    want = KA.segment(window, rect_size)
    for rect in ((4, 2) + rect_size, (0, 0) + rect_size):
        o = roi(window=window, rect=rect)
        n = lib.p264hip_roi_aa_segment_words(C.byref(o), C.byref(r))
        assert n == want.size and n % 4 == 0, (n, want.size)
        got = np.full(n + 8, 0xA5A5A5A5, np.uint32)
        assert lib.p264hip_roi_aa_segment(C.byref(o), C.byref(r), got.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        assert np.all(got[n:] == 0xA5A5A5A5)
        bad = np.flatnonzero(got[:n] != want)
        assert bad.size == 0, "word %d of %d: %08x, want %08x" % (bad[0], n, got[bad[0]], want[bad[0]])
    # the whole output where the rectangle is all 0
    whole = desc(size=rect_size)
    o = roi(window=window)
    assert lib.p264hip_roi_aa_segment_words(C.byref(o), C.byref(whole)) == want.size
    got = np.zeros(want.size, np.uint32)
    assert lib.p264hip_roi_aa_segment(C.byref(o), C.byref(whole), got.ctypes.data_as(C.POINTER(C.c_uint32))) == 0 and np.array_equal(got, want)


def test_the_segment_helpers_refuse(lib):
    r = desc(size=(34, 18))
    words = (C.c_uint32 * 4096)()
    assert lib.p264hip_roi_aa_segment_words(None, C.byref(r)) == EINVAL and lib.p264hip_roi_aa_segment_words(C.byref(roi()), None) == EINVAL
    assert lib.p264hip_roi_aa_segment(C.byref(roi()), C.byref(r), None) == EINVAL
    for o in (roi(window=(0, 0, 66, 2), rect=(0, 0, 2, 2)), roi(window=(0, 0, 3, 2)), roi(window=(0, 0, 0, 2)), roi(rect=(0, 0, 3, 2)), roi(window=(-2, 0, 4, 4))):
        assert lib.p264hip_roi_aa_segment_words(C.byref(o), C.byref(r)) == EINVAL and lib.p264hip_roi_aa_segment(C.byref(o), C.byref(r), words) == EINVAL


def test_resize_aa_taps_is_the_shared_text(lib):
    """p264hip_resize_aa_taps calls the text the segment is made with: the same first, count and weights"""
    for S, D in ((30, 62), (30, 30), (60, 30), (70, 22), (64, 2), (1080, 34)):
        first, count, w = (C.c_int32 * D)(), (C.c_int32 * D)(), (C.c_uint16 * (D * 64))()
        assert lib.p264hip_resize_aa_taps(S, D, first, count, w) == 0
        f, c, ww = A.aa_taps(S, D)
        assert list(first) == list(f) and list(count) == list(c) and np.array_equal(np.array(w).reshape(D, 64), ww)


# ---- the model against the models it is built on
@pytest.fixture(scope="module")
def frame():
    g = np.random.default_rng(2670)
    return g.integers(0, 256, (48, 80), np.uint8), g.integers(0, 256, (24, 40), np.uint8), g.integers(0, 256, (24, 40), np.uint8)


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_the_model_with_whole_rectangles_is_the_resize_aa_model(frame, fmt, dtype):
    scale, bias = ((1 / 255,) * 3, (-0.5, 0.0, 0.25)) if dtype != "u8" else (None, None)
    matrix, full = ("bt709", True) if fmt.startswith("rgb") else ("bt601", False)
    for window, size in (((2, 2, 62, 30), (34, 18)), ((0, 0, 80, 48), (162, 98)), ((6, 46, 2, 2), (6, 70)), ((16, 10, 48, 22), (48, 22)), ((0, 0, 64, 32), (2, 2))):
        tight = R.tight_pitch(fmt, size[0], dtype)
        for pitch, stride, offset in ((0, 0, 0), (tight + 16, R.frame_bytes(fmt, size[0], size[1], dtype, tight + 16) + 8, 4)):
            want = A.expected_aa([frame] * 3, fmt, window, size, dtype, scale, bias, matrix, full, pitch, stride, offset)
            rows = [(0, 0) + window, (0, 0) + window + (0, 0, 0, 0), (0, 0) + window + (0, 0) + size]       # the three ways to say "whole"
            got = KA.expected(rows, {(0, 0): frame}, size, fmt, dtype, (1, 2, 3), scale, bias, matrix, full, pitch, stride, offset)
            assert np.array_equal(got, want), (fmt, dtype, window, size, pitch)


def test_a_rectangle_of_the_windows_size_pastes_the_window(frame):
    y, u, v = frame
    for window, at, size in (((16, 10, 48, 22), (2, 4), (54, 30)), ((0, 0, 80, 48), (0, 0), (80, 48)), ((78, 46, 2, 2), (32, 16), (34, 18))):
        x0, y0, w, h = window
        vy, vu, vv = KA.virtual_planes(frame, window, at + (w, h), size, (9, 99, 199))
        assert np.array_equal(vy[at[1]:at[1] + h, at[0]:at[0] + w], y[y0:y0 + h, x0:x0 + w])
        assert np.array_equal(vu[at[1] // 2:(at[1] + h) // 2, at[0] // 2:(at[0] + w) // 2], u[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
        assert np.array_equal(vv[at[1] // 2:(at[1] + h) // 2, at[0] // 2:(at[0] + w) // 2], v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
        mask = np.ones(vy.shape, bool)
        mask[at[1]:at[1] + h, at[0]:at[0] + w] = False
        assert np.all(vy[mask] == 9) and np.all(vu[mask[::2, ::2]] == 99) and np.all(vv[mask[::2, ::2]] == 199)
        # ... and so it is the filter-0 model's picture
        for a, b in zip((vy, vu, vv), K.virtual_planes(frame, window, at + (w, h), size, (9, 99, 199))):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_bytes_outside_the_rectangle_are_those_of_the_filter_0_call(frame, fmt, dtype):
    size, rect = (34, 18), (6, 4, 22, 10)
    scale, bias = ((1 / 255,) * 3, (0.0,) * 3) if dtype != "u8" else (None, None)
    for fill in ((16, 128, 128), (235, 16, 240), (0, 255, 0)):
        row = [(0, 0, 2, 2, 62, 30) + rect]
        plain = K.expected(row, {(0, 0): frame}, size, fmt, dtype, fill, scale, bias)
        got = KA.expected(row, {(0, 0): frame}, size, fmt, dtype, fill, scale, bias)
        # which bytes belong to samples outside the rectangle: those the filter-0 model writes the same for two opposite windows
        const = (np.full((48, 80), 3, np.uint8), np.full((24, 40), 250, np.uint8), np.full((24, 40), 7, np.uint8))
        a = K.expected(row, {(0, 0): const}, size, fmt, dtype, fill, scale, bias)
        b = K.expected(row, {(0, 0): tuple(255 - c for c in const)}, size, fmt, dtype, fill, scale, bias)
        bits = {"u8": np.uint8, "f16": np.uint16, "f32": np.uint32}[dtype]                         # (element by element: single bytes of two floats may agree)
        outside = np.repeat(a.view(bits) == b.view(bits), np.dtype(bits).itemsize)
        if fmt in ("i420", "nv12", "rgbp") and dtype == "u8":
            assert outside.sum() == plain.size - {"i420": 22 * 10 * 3 // 2, "nv12": 22 * 10 * 3 // 2, "rgbp": 3 * 22 * 10}[fmt]
        assert np.array_equal(got[outside], plain[outside]) and not np.array_equal(got, plain), (fmt, dtype, fill)


def test_abi_and_signatures(lib):
    for f in ("p264hip_rois_aa_frame_bytes", "p264hip_rois_aa_check", "p264hip_export_rois_aa", "p264hip_roi_aa_segment_words", "p264hip_roi_aa_segment", "p264hip_roi_aa_tile_width"):
        assert hasattr(lib, f), f
    assert lib.p264hip_export_rois_aa.argtypes == lib.p264hip_export_rois.argtypes and lib.p264hip_rois_aa_check.argtypes == lib.p264hip_rois_check.argtypes
    a, b = (inspect.signature(getattr(p264decoder_amd.HipReconstructor, f)) for f in ("export_rois_aa", "export_rois"))
    assert str(a) == str(b)
    sig = inspect.signature(p264decoder_amd.Pipeline.export_last_rois)
    assert sig.parameters["filter"].default == "bilinear" and sig.parameters["filter"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_kernels_are_in_the_code_object_without_spills_or_scratch(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for k in KERNELS:
        assert k in res, sorted(res)
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
        assert r["group_segment_fixed_size"] == (512 if "rgb" in k else 0), (k, r)                  # (the t of a tile are dynamic)
