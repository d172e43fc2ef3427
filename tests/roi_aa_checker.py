"""A numpy model of the export of per-picture windows with the ANTIALIASED filter (include/p264hip.h: p264hip_export_rois_aa), written
from its description alone: tests/roi_checker.py's virtual picture with tests/resize_aa_checker.py's resize_plane_aa in place of
resize_plane, handed to resize_checker.put_frame with the window (0, 0, W, H) and the size (W, H) - D == S returns the source there,
so the layout, RGB and float steps are the existing model's.  Also the segment of an ROI and the two closed-form bounds, from the
header's words.  The checker of tests/test_roi_aa_cpu.py and tests/test_gpu_roi_aa*.py - never the product."""
import numpy as np

from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests.roi_checker import FILL, split

_virtual = {}
_taps = {}


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
    assert cw <= 32 * dw and ch <= 32 * dh
    y, u, v = planes
    out = [np.full((H, W), fill[0], np.uint8), np.full((H // 2, W // 2), fill[1], np.uint8), np.full((H // 2, W // 2), fill[2], np.uint8)]
    out[0][dt:dt + dh, dl:dl + dw] = A.resize_plane_aa(y[y0:y0 + ch, x0:x0 + cw], dw, dh)[0]
    for i, c in ((1, u), (2, v)):
        out[i][dt // 2:(dt + dh) // 2, dl // 2:(dl + dw) // 2] = A.resize_plane_aa(c[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], dw // 2, dh // 2)[0]
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


# ---- the segment of an ROI and its bounds
def taps(S, D):
    """resize_aa_checker.aa_taps, kept"""
    if (S, D) not in _taps:
        _taps[(S, D)] = A.aa_taps(S, D)
    return _taps[(S, D)]


def stride(S, D):
    """16-bit weights of a row of the axis S -> D: 2 for S <= D, min(64, ceil(2 S / D)) rounded up to even otherwise"""
    return 2 if S <= D else (min(64, -(-2 * S // D)) + 1) & ~1


def span_bound(S, D, tw):
    """source samples a tile of tw destination samples spans at most, wherever it begins"""
    return -(-(tw - 1) * S // D) + stride(S, D) + 1


def pad4(n):
    return (n + 3) & ~3


def axis_words(origin, S, D):
    """an axis of a segment as uint32 words: pad4(D) words first | count << 16, first a coordinate of the frame, the padding the last
    one; then D rows of `stride` 16-bit weights, 0 behind the count, padded with 0 to a multiple of 4 words"""
    first, count, w = taps(S, D)
    st = stride(S, D)
    assert count.max() <= st
    pos = np.empty(pad4(D), np.uint32)
    pos[:D] = (origin + first) | count << 16
    pos[D:] = pos[D - 1]
    rows = np.zeros(2 * pad4(D * st // 2), np.uint16)
    rows[:D * st] = w[:, :st].astype(np.uint16).reshape(-1)
    return np.concatenate([pos, rows.view(np.uint32)])


def segment(window, rect_size):
    """the segment of a window (left, top, width, height) into a rectangle of (dw, dh): x luma, y luma, x chroma, y chroma"""
    left, top, width, height = window
    dw, dh = rect_size
    return np.concatenate([axis_words(left, width, dw), axis_words(top, height, dh), axis_words(left // 2, width // 2, dw // 2), axis_words(top // 2, height // 2, dh // 2)])
