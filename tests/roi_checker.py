"""A numpy model of the export of per-picture windows into rectangles of the output (include/p264hip.h: p264hip_roi_t), written from
its description alone.  Per ROI: planes full of the fill, tests/resize_checker.py's resize_plane of the window's three planes pasted
into the rectangle, and the virtual planes handed to resize_checker.put_frame with the window (0, 0, W, H) and the size (W, H) - D == S
returns the source, so the layout, RGB and float steps are the existing model's.  The checker of tests/test_roi_cpu.py and
tests/test_gpu_roi*.py - never the product."""
import numpy as np

from tests import resize_checker as R

FILL = (16, 128, 128)
_virtual = {}


def split(roi):
    """a row (stream, slot, left, top, width, height[, dst_left, dst_top, dst_width, dst_height]) -> ((stream, slot), window, rectangle or None)"""
    roi = tuple(int(v) for v in roi)
    assert len(roi) in (6, 10), roi
    rect = roi[6:] if len(roi) == 10 and any(roi[6:]) else None
    return roi[:2], roi[2:6], rect


def virtual_planes(planes, window, rect, size, fill=FILL, key=None):
    """(Y, U, V) of the virtual W x H picture; key: what names `planes` in the cache (None: not cached)"""
    W, H = size
    rect = (0, 0, W, H) if rect is None else tuple(rect)
    k = (key, tuple(window), rect, (W, H), tuple(fill))
    if key is not None and k in _virtual:
        return _virtual[k]
    x0, y0, cw, ch = window
    dl, dt, dw, dh = rect
    assert not (x0 | y0 | cw | ch | dl | dt | dw | dh) & 1 and cw > 0 and ch > 0 and dw >= 2 and dh >= 2 and dl + dw <= W and dt + dh <= H
    y, u, v = planes
    out = [np.full((H, W), fill[0], np.uint8), np.full((H // 2, W // 2), fill[1], np.uint8), np.full((H // 2, W // 2), fill[2], np.uint8)]
    out[0][dt:dt + dh, dl:dl + dw] = R.resize_plane(y[y0:y0 + ch, x0:x0 + cw], dw, dh)[0]
    for i, c in ((1, u), (2, v)):
        out[i][dt // 2:(dt + dh) // 2, dl // 2:(dl + dw) // 2] = R.resize_plane(c[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], dw // 2, dh // 2)[0]
    out = tuple(out)
    if key is not None:
        _virtual[k] = out
    return out


def put_roi(dst, planes, window, rect, size, fmt, dtype="u8", fill=FILL, scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, key=None):
    """One output picture into dst (a uint8 array): only the bytes the layout names are written."""
    W, H = size
    R.put_frame(dst, virtual_planes(planes, window, rect, size, fill, key), fmt, (0, 0, W, H), (W, H), dtype, scale, bias, matrix, full_range, pitch)


def expected(rois, frames, size, fmt, dtype="u8", fill=FILL, scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, frame_stride=0, offset=0,
             total=None, prefill=0xA5, tag=None):
    """The whole destination: `total` bytes of `prefill` with output picture i of `rois` at offset + i * frame_stride.  frames: the
    (y, u, v) of every (stream, slot) a ROI names; tag: what names `frames` in the cache (None: nothing is cached)."""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    stride = frame_stride or per
    need = offset + (len(rois) - 1) * stride + per
    dst = np.full(total if total is not None else need, prefill, np.uint8)
    assert dst.size >= need
    for i, roi in enumerate(rois):
        pic, window, rect = split(roi)
        put_roi(dst[offset + i * stride:], frames[pic], window, rect, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch,
                key=None if tag is None else (tag, pic))
    return dst
