"""The model of the export from an ROI list in device memory (include/p264hip.h: p264hip_export_rois_device), written from its
description alone: the STATUS of an ROI restated in Python integers from the header's table - never through p264hip_roi_status -, and
the expected destination: tests/roi_checker.py's / tests/roi_aa_checker.py's picture for every ROI whose status is 0, the prefill
over the whole byte range of every other.  The checker of tests/test_roi_device_cpu.py and tests/test_gpu_roi_device*.py - never the
product."""
import numpy as np

from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K

(OK, UNUSED, BAD_PICTURE, NO_PICTURE, WINDOW_EMPTY, WINDOW_ODD, WINDOW_OUTSIDE, RECT_SMALL, RECT_ODD, RECT_OUTSIDE, REDUCTION) = range(11)


def status(roi, size, filter, frame, store, max_reduction=0, table=None):
    """the status of one row (stream, slot, left, top, width, height, dst_left, dst_top, dst_width, dst_height) of Python integers in
    a size = (W, H) output with filter 0 / 2, a frame = (width, height) in samples and a store = (n_streams, slots); table: the slot
    of every stream (-1: no picture) that slot -1 stands for, None: slot -1 is out of range"""
    stream, slot, left, top, width, height, dl, dt, dw, dh = (int(v) for v in roi)
    W, H = size
    n_streams, slots = store
    if stream < 0 or stream >= n_streams:
        return BAD_PICTURE
    if slot == -1 and table is not None:
        slot = int(table[stream])
        if slot < 0:
            return NO_PICTURE
    if slot < 0 or slot >= slots:
        return BAD_PICTURE
    if left < 0 or top < 0 or width < 1 or height < 1:
        return WINDOW_EMPTY
    if (left | top | width | height) & 1:
        return WINDOW_ODD
    if left + width > frame[0] or top + height > frame[1]:
        return WINDOW_OUTSIDE
    whole = dl == dt == dw == dh == 0
    if not whole:
        if dl < 0 or dt < 0 or dw < 2 or dh < 2:
            return RECT_SMALL
        if (dl | dt | dw | dh) & 1:
            return RECT_ODD
        if dl + dw > W or dt + dh > H:
            return RECT_OUTSIDE
    if filter == 2:
        m = max_reduction or 32
        if width > m * (W if whole else dw) or height > m * (H if whole else dh):
            return REDUCTION
    return OK


def statuses(rois, size, filter, frame, store, max_reduction=0, table=None, count=None):
    """the status words of a call: rows from the count (clamped into 0 .. n; None: n) on are UNUSED"""
    n = len(rois)
    used = n if count is None else min(max(int(count), 0), n)
    return [status(r, size, filter, frame, store, max_reduction, table) if i < used else UNUSED for i, r in enumerate(rois)]


def expected(rois, st, frames, size, fmt, filter=0, dtype="u8", fill=K.FILL, scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, frame_stride=0,
             offset=0, total=None, prefill=0xA5, tag=None, table=None):
    """The whole destination: `total` bytes of `prefill` with output picture i at offset + i * frame_stride where st[i] is 0 - and
    nothing where it is not.  frames: the (y, u, v) of every (stream, slot) a valid ROI names."""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    stride = frame_stride or per
    need = offset + (len(rois) - 1) * stride + per
    dst = np.full(total if total is not None else need, prefill, np.uint8)
    assert dst.size >= need and len(st) == len(rois)
    put = KA.put_roi if filter == 2 else K.put_roi
    for i, roi in enumerate(rois):
        if st[i] != OK:
            continue
        roi = [int(v) for v in roi]
        if roi[1] == -1:
            roi[1] = int(table[roi[0]])
        pic, window, rect = K.split(roi)
        put(dst[offset + i * stride:], frames[pic], window, rect, size, fmt, dtype, fill, scale, bias, matrix, full_range, pitch,
            key=None if tag is None else (tag, pic))
    return dst
