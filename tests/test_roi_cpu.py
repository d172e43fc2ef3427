"""The host side of the export of per-picture windows into rectangles of the output (include/p264hip.h: p264hip_roi_t), no GPU: the
refusals of p264hip_rois_check / p264hip_rois_frame_bytes, the numpy model of tests/roi_checker.py against the resize model it is
built on, letterbox(), the ctypes mirror and the Python signatures, and the nine kernels in the code object."""
import ctypes as C
import inspect

import numpy as np
import pytest

import p264decoder_amd
from p264decoder_amd import _native as N
from tests import resize_checker as R
from tests import roi_checker as K

EINVAL = -1
MB_W, MB_H, STREAMS, SLOTS = 5, 3, 3, 2                     # the 80 x 48 frame of tests/test_gpu_resize.py
INSTANCES = [("i420", "u8"), ("nv12", "u8"), ("rgb24", "u8"), ("rgbp", "u8"), ("rgb24", "f16"), ("rgbp", "f16"), ("rgb24", "f32"), ("rgbp", "f32")]
KERNELS = ("k_roi_taps", "k_roi_i420", "k_roi_nv12", "k_roi_rgb24_u8", "k_roi_rgb24_f16", "k_roi_rgb24_f32", "k_roi_rgbp_u8", "k_roi_rgbp_f16", "k_roi_rgbp_f32")
FILL_WORD = 16 | 128 << 8 | 128 << 16


def desc(fmt="rgbp", size=(34, 18), crop=(0, 0, 2, 2), **kw):
    return N.resize_desc(fmt, size, crop, None, **kw)


def roi(stream=0, slot=0, window=(2, 2, 62, 30), rect=(0, 0, 0, 0)):
    return N.Roi(stream, slot, *window, *rect)


def check(lib, rois, r, fill=FILL_WORD, n=None, mb=(MB_W, MB_H), store=(STREAMS, SLOTS)):
    arr = (N.Roi * len(rois))(*rois) if rois is not None else None
    return lib.p264hip_rois_check(arr, len(rois) if n is None else n, C.byref(r) if r is not None else None, fill, mb[0], mb[1], store[0], store[1])


def test_the_refusals_of_the_roi_list(lib):
    good = roi()
    assert check(lib, [good], desc()) == 0
    # (refused, the accepted case beside it)
    pairs = [
        # each odd or non-positive window member
        (roi(window=(1, 2, 62, 30)), roi(window=(2, 2, 62, 30))), (roi(window=(2, 1, 62, 30)), roi(window=(2, 0, 62, 30))),
        (roi(window=(2, 2, 61, 30)), roi(window=(2, 2, 60, 30))), (roi(window=(2, 2, 62, 29)), roi(window=(2, 2, 62, 28))),
        (roi(window=(2, 2, 0, 30)), roi(window=(2, 2, 2, 30))), (roi(window=(2, 2, 62, 0)), roi(window=(2, 2, 62, 2))),
        (roi(window=(2, 2, -2, 30)), roi(window=(2, 2, 2, 30))), (roi(window=(2, 2, 62, -2)), roi(window=(2, 2, 62, 2))),
        (roi(window=(-2, 2, 62, 30)), roi(window=(0, 2, 62, 30))), (roi(window=(2, -2, 62, 30)), roi(window=(2, 0, 62, 30))),
        # a window leaving the 80 x 48 frame on each side
        (roi(window=(0, 0, 82, 48)), roi(window=(0, 0, 80, 48))), (roi(window=(0, 0, 80, 50)), roi(window=(0, 0, 80, 48))),
        (roi(window=(20, 0, 62, 30)), roi(window=(18, 0, 62, 30))), (roi(window=(0, 20, 62, 30)), roi(window=(0, 18, 62, 30))),
        (roi(window=(80, 0, 2, 2)), roi(window=(78, 0, 2, 2))), (roi(window=(0, 48, 2, 2)), roi(window=(0, 46, 2, 2))),
        # a rectangle with one odd member, or leaving the 34 x 18 output on each side
        (roi(rect=(1, 2, 30, 14)), roi(rect=(2, 2, 30, 14))), (roi(rect=(2, 1, 30, 14)), roi(rect=(2, 2, 30, 14))),
        (roi(rect=(2, 2, 29, 14)), roi(rect=(2, 2, 30, 14))), (roi(rect=(2, 2, 30, 13)), roi(rect=(2, 2, 30, 14))),
        (roi(rect=(6, 0, 30, 18)), roi(rect=(4, 0, 30, 18))), (roi(rect=(0, 6, 34, 14)), roi(rect=(0, 4, 34, 14))),
        (roi(rect=(0, 0, 36, 18)), roi(rect=(0, 0, 34, 18))), (roi(rect=(0, 0, 34, 20)), roi(rect=(0, 0, 34, 18))),
        (roi(rect=(-2, 0, 34, 18)), roi(rect=(0, 0, 34, 18))), (roi(rect=(0, -2, 34, 18)), roi(rect=(0, 0, 34, 18))),
        (roi(rect=(34, 0, 2, 2)), roi(rect=(32, 0, 2, 2))), (roi(rect=(0, 18, 2, 2)), roi(rect=(0, 16, 2, 2))),
        # a rectangle with some but not all members 0
        (roi(rect=(0, 0, 34, 0)), roi(rect=(0, 0, 34, 18))), (roi(rect=(0, 0, 0, 18)), roi(rect=(0, 0, 34, 18))),
        (roi(rect=(2, 0, 0, 0)), roi(rect=(0, 0, 0, 0))), (roi(rect=(0, 2, 0, 0)), roi(rect=(0, 0, 0, 0))),
        (roi(rect=(0, 0, 0, 2)), roi(rect=(0, 0, 2, 2))), (roi(rect=(0, 0, 2, 0)), roi(rect=(0, 0, 2, 2))),
        # a stream or slot out of range
        (roi(stream=STREAMS), roi(stream=STREAMS - 1)), (roi(stream=-1), roi(stream=0)), (roi(slot=SLOTS), roi(slot=SLOTS - 1)), (roi(slot=-1), roi(slot=0)),
    ]
    for i, (bad, ok) in enumerate(pairs):
        assert check(lib, [bad], desc()) == EINVAL, i
        assert check(lib, [good, good, bad], desc()) == EINVAL, i          # ... wherever it stands in the list
        assert check(lib, [ok], desc()) == 0, i
        assert check(lib, [good, ok, good], desc()) == 0, i
    # n = 0, a null pointer, no frame, no frame store
    assert check(lib, [good], desc(), n=0) == EINVAL and check(lib, [good], desc(), n=-1) == EINVAL
    assert lib.p264hip_rois_check(None, 1, C.byref(desc()), FILL_WORD, MB_W, MB_H, STREAMS, SLOTS) == EINVAL
    assert check(lib, [good], None) == EINVAL
    for mb in ((0, 3), (5, 0), (-1, 3)):
        assert check(lib, [roi(window=(0, 0, 2, 2))], desc(), mb=mb) == EINVAL
    for store in ((0, 2), (3, 0)):
        assert check(lib, [good], desc(), store=store) == EINVAL
    # a fill with bit 24 set (and above)
    for fill, ok in ((1 << 24, False), (1 << 31, False), (0xffffff, True), (0, True), (0x1000000 | FILL_WORD, False)):
        assert (check(lib, [good], desc(), fill=fill) == 0) == ok, hex(fill)
    # the whole frame into the whole output, the smallest window into the smallest rectangle at the far corner
    assert check(lib, [roi(2, 1, (0, 0, 80, 48)), roi(0, 0, (78, 46, 2, 2), (32, 16, 2, 2))], desc()) == 0


def test_the_refusals_of_the_description(lib):
    fb = lib.p264hip_rois_frame_bytes
    assert fb(None) == EINVAL
    inf, nan = float("inf"), float("nan")
    pairs = [
        # the filter: 2 is the antialiased one, 1 is not assigned
        (desc(filter=2), desc(filter=0)), (desc(filter=1), desc(filter=0)), (desc(filter=-1), desc(filter=0)),
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
        assert fb(C.byref(bad)) == EINVAL and check(lib, one, bad) == EINVAL, i
        assert fb(C.byref(good)) > 0 and check(lib, one, good) == 0, i
    # a frame_stride below the picture's bytes, or no multiple of the element size
    per = 3 * 34 * 18
    for r, stride, ok in ((desc(), per - 1, False), (desc(), per, True), (desc(), -8, False), (desc(dtype="f16"), 2 * per + 2, True), (desc(dtype="f16"), 2 * per + 1, False),
                          (desc(dtype="f32"), 4 * per + 6, False), (desc(dtype="f32"), 4 * per + 8, True)):
        r.frame_stride = stride
        assert fb(C.byref(r)) > 0 and (check(lib, one, r) == 0) == ok, (r.dtype, stride)


def test_the_crop_fields_are_not_read(lib):
    """any crop_* values are accepted and change nothing: windows p264hip_resize_check refuses, odd, negative, outside every frame"""
    for fmt, dtype in INSTANCES:
        want = R.frame_bytes(fmt, 34, 18, dtype)
        for crop in ((0, 0, 2, 2), (1, 1, 1, 1), (-5, -7, 0, 0), (0, 0, 80, 50), (1 << 30, 1 << 30, 1 << 30, 1 << 30), (0, 0, -2, -2), (0, 0, 1920, 1080)):
            r = desc(fmt, dtype=dtype, crop=crop)
            assert lib.p264hip_rois_frame_bytes(C.byref(r)) == want, (fmt, dtype, crop)
            assert check(lib, [roi()], r) == 0, (fmt, dtype, crop)
            plain = desc(fmt, dtype=dtype, crop=(0, 0, 80, 48))
            assert lib.p264hip_resize_frame_bytes(C.byref(plain)) == want


@pytest.fixture(scope="module")
def frame():
    g = np.random.default_rng(2660)
    return g.integers(0, 256, (48, 80), np.uint8), g.integers(0, 256, (24, 40), np.uint8), g.integers(0, 256, (24, 40), np.uint8)


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_the_model_with_whole_rectangles_is_the_resize_model(frame, fmt, dtype):
    scale, bias = ((1 / 255,) * 3, (-0.5, 0.0, 0.25)) if dtype != "u8" else (None, None)
    matrix, full = ("bt709", True) if fmt.startswith("rgb") else ("bt601", False)
    for window, size in (((2, 2, 62, 30), (34, 18)), ((0, 0, 80, 48), (162, 98)), ((6, 46, 2, 2), (6, 70)), ((16, 10, 48, 22), (48, 22))):
        tight = R.tight_pitch(fmt, size[0], dtype)
        for pitch, stride, offset in ((0, 0, 0), (tight + 16, R.frame_bytes(fmt, size[0], size[1], dtype, tight + 16) + 8, 4)):
            want = R.expected([frame] * 3, fmt, window, size, dtype, scale, bias, matrix, full, pitch, stride, offset)
            rows = [(0, 0) + window, (0, 0) + window + (0, 0, 0, 0), (0, 0) + window + (0, 0) + size]       # the three ways to say "whole"
            got = K.expected(rows, {(0, 0): frame}, size, fmt, dtype, (1, 2, 3), scale, bias, matrix, full, pitch, stride, offset)
            assert np.array_equal(got, want), (fmt, dtype, window, size, pitch)


def test_a_rectangle_of_the_windows_size_pastes_the_window(frame):
    y, u, v = frame
    for window, at, size in (((16, 10, 48, 22), (2, 4), (54, 30)), ((0, 0, 80, 48), (0, 0), (80, 48)), ((78, 46, 2, 2), (32, 16), (34, 18))):
        x0, y0, w, h = window
        vy, vu, vv = K.virtual_planes(frame, window, at + (w, h), size, (9, 99, 199))
        assert np.array_equal(vy[at[1]:at[1] + h, at[0]:at[0] + w], y[y0:y0 + h, x0:x0 + w])
        assert np.array_equal(vu[at[1] // 2:(at[1] + h) // 2, at[0] // 2:(at[0] + w) // 2], u[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
        assert np.array_equal(vv[at[1] // 2:(at[1] + h) // 2, at[0] // 2:(at[0] + w) // 2], v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
        mask = np.ones(vy.shape, bool)
        mask[at[1]:at[1] + h, at[0]:at[0] + w] = False
        assert np.all(vy[mask] == 9) and np.all(vu[mask[::2, ::2]] == 99) and np.all(vv[mask[::2, ::2]] == 199)


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_bytes_outside_the_rectangle_are_the_export_of_a_constant_picture(frame, fmt, dtype):
    size, rect = (34, 18), (6, 4, 22, 10)
    scale, bias = ((1 / 255,) * 3, (0.0,) * 3) if dtype != "u8" else (None, None)
    for fill in ((16, 128, 128), (235, 16, 240), (0, 255, 0)):
        const = (np.full((18, 34), fill[0], np.uint8), np.full((9, 17), fill[1], np.uint8), np.full((9, 17), fill[2], np.uint8))
        flat = R.expected([const], fmt, (0, 0, 34, 18), size, dtype, scale, bias)
        got = K.expected([(0, 0, 2, 2, 62, 30) + rect], {(0, 0): frame}, size, fmt, dtype, fill, scale, bias)
        # which bytes belong to samples outside the rectangle: those the same call leaves alone when the window itself is the constant
        marked = K.expected([(0, 0, 0, 0, 34, 18) + rect], {(0, 0): tuple(255 - c for c in const)}, size, fmt, dtype, fill, scale, bias)
        bits = {"u8": np.uint8, "f16": np.uint16, "f32": np.uint32}[dtype]                         # (element by element: single bytes of two floats may agree)
        outside = np.repeat(marked.view(bits) == flat.view(bits), np.dtype(bits).itemsize)
        if fmt in ("i420", "nv12", "rgbp") and dtype == "u8":
            assert outside.sum() == flat.size - {"i420": 22 * 10 * 3 // 2, "nv12": 22 * 10 * 3 // 2, "rgbp": 3 * 22 * 10}[fmt]
        assert np.array_equal(got[outside], flat[outside]) and not np.array_equal(got, flat), (fmt, dtype, fill)


def test_letterbox():
    lb = N.letterbox
    assert p264decoder_amd.letterbox is lb
    assert lb(1920, 1080, 640, 640) == (0, 140, 640, 360)
    assert lb(1080, 1920, 640, 640) == (140, 0, 360, 640)
    assert lb(80, 48, 34, 18) == (2, 0, 30, 18) and lb(640, 640, 640, 640) == (0, 0, 640, 640) and lb(1920, 1080, 224, 224) == (0, 48, 224, 126)
    assert lb(4000, 2, 16, 16) == (0, 6, 16, 2) and lb(2, 4000, 16, 16) == (6, 0, 2, 16)
    g = np.random.default_rng(2661)
    for w, h, W, H in zip(*(2 * g.integers(1, n, 4000) for n in (2048, 2048, 512, 512))):
        w, h, W, H = int(w), int(h), int(W), int(H)
        l, t, dw, dh = lb(w, h, W, H)
        assert not (l | t | dw | dh) & 1 and l >= 0 and t >= 0 and dw >= 2 and dh >= 2 and l + dw <= W and t + dh <= H, (w, h, W, H)
        assert dw == W or dh == H
        assert abs(l - (W - dw - l)) <= 2 and abs(t - (H - dh - t)) <= 2                       # centred to the even sample
        if dw == W and dh != H:
            assert abs(dh * w - h * W) <= 2 * w or dh == 2, (w, h, W, H)                           # within 2 of the exact ratio (or the floor of 2)
        elif dh == H and dw != W:
            assert abs(dw * h - w * H) <= 2 * h or dw == 2, (w, h, W, H)


def test_abi_mirror_and_signatures(lib):
    import os
    import subprocess
    import tempfile
    names = [n for n, _ in N.Roi._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "p264pipe.h"\nint main(void) { printf("%zu %zu %d", sizeof(p264hip_roi_t), sizeof(p264hip_resize_t), P264HIP_ROI_SCRATCH_BYTES);\n'
           + "".join('printf(" %%zu", offsetof(p264hip_roi_t, %s));\n' % n for n in names) + 'printf("\\n"); return 0; }\n')
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I" + inc, os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(td, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert out[0] == C.sizeof(N.Roi) == 40 and out[1] == C.sizeof(N.Resize) == 80 and out[2] == N.ROI_SCRATCH_BYTES
    assert out[3:] == [getattr(N.Roi, n).offset for n in names] == list(range(0, 40, 4))
    for f in ("p264hip_rois_frame_bytes", "p264hip_rois_check", "p264hip_export_rois", "p264pipe_export_last_rois"):
        assert hasattr(lib, f)
    assert lib.p264hip_export_rois.argtypes[1:] == [C.POINTER(N.Roi), C.c_int, C.POINTER(N.Resize), C.c_uint32, C.c_void_p, C.c_size_t]
    assert lib.p264pipe_export_last_rois.argtypes[1:] == lib.p264hip_export_rois.argtypes[1:]
    sig = inspect.signature(p264decoder_amd.HipReconstructor.export_rois)
    assert list(sig.parameters) == ["self", "rois", "size", "fmt", "dtype", "fill", "scale", "bias", "matrix", "full_range", "pitch", "frame_stride", "out", "sync"]
    assert [sig.parameters[k].default for k in ("fmt", "dtype", "fill", "matrix", "full_range", "pitch", "frame_stride", "out", "sync")] == ["rgbp", "u8", (16, 128, 128), "bt601", False, 0, 0, None, True]
    sig = inspect.signature(p264decoder_amd.Pipeline.export_last_rois)
    assert list(sig.parameters)[:6] == ["self", "rois", "size", "fmt", "dtype", "fill"] and sig.parameters["fill"].default == (16, 128, 128)


def test_six_and_ten_columns():
    six, n = N.roi_array([(1, 0, 2, 4, 62, 30), (2, 1, 0, 0, 80, 48)])
    ten, m = N.roi_array([(1, 0, 2, 4, 62, 30, 0, 0, 0, 0), (2, 1, 0, 0, 80, 48, 0, 0, 0, 0)])
    assert n == m == 2 and bytes(six) == bytes(ten)
    assert [getattr(six[0], f) for f, _ in N.Roi._fields_] == [1, 0, 2, 4, 62, 30, 0, 0, 0, 0]
    mixed, n = N.roi_array([(1, 0, 2, 4, 62, 30), (2, 1, 0, 0, 80, 48, 6, 0, 22, 18)])
    assert n == 2 and [getattr(mixed[1], f) for f, _ in N.Roi._fields_] == [2, 1, 0, 0, 80, 48, 6, 0, 22, 18] and mixed[0].dst_width == 0
    a6 = np.array([(1, 0, 2, 4, 62, 30), (2, 1, 0, 0, 80, 48)], np.int32)
    a10 = np.concatenate([a6, np.array([[0, 0, 0, 0], [6, 0, 22, 18]], np.int32)], axis=1)
    assert bytes(N.roi_array(a6)[0]) == bytes(six) and bytes(N.roi_array(a10)[0]) == bytes(mixed)
    # the pipeline's rows carry no slot: it becomes -1
    five, n = N.roi_array([(1, 2, 4, 62, 30), (2, 0, 0, 80, 48, 6, 0, 22, 18)], head=1)
    assert [getattr(five[1], f) for f, _ in N.Roi._fields_] == [2, -1, 0, 0, 80, 48, 6, 0, 22, 18] and five[0].slot == -1 and five[0].stream == 1
    for bad in ([(1, 0, 2, 4, 62)], [(1, 0, 2, 4, 62, 30, 0)], np.zeros((2, 7), np.int32), np.zeros((2, 6), np.float32)):
        with pytest.raises(ValueError):
            N.roi_array(bad)
    assert N.fill_word((16, 128, 128)) == FILL_WORD and N.fill_word((0, 255, 0)) == 0xff00
    with pytest.raises(ValueError):
        N.fill_word((256, 0, 0))


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
