"""The staging ring of the device export with calls IN FLIGHT.  Every export road writes its call's table - frame indices, tap
tables, ROI descriptors - into one of BATCH_RING pinned buffers and copies it to its device twin on the context's stream; a buffer
is written again only when the copy that last used it is done, and the ring grows when a call's table exceeds it (csrc/hip/p264hip.hip).
The other export tests wait after every call.  This one queues nine with sync=False, rotating over the five roads - export_resized
with the bilinear and the antialiased filter, export_rois, export_rois_aa, export_frames - so that every buffer of the ring is
taken again with the stream busy, and waits once.  The context is fresh: its first call sizes the ring (a 2 x 2 output of one
picture, 20 words, gives n + n // 2 + 16 = 46), the next four fit that, and the sixth - 40 ROIs, 320 words of descriptors - makes
the ring grow behind five queued calls.  Every destination was prefilled and is compared whole, byte for byte, with the numpy
checkers of the five roads applied to the read_frame planes - never with another call of the library."""
import numpy as np
import pytest

from tests import export_checker as X
from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K
from tests.device_mem import DeviceBuffer
from tests.hip_harness import reconstructor
from tests.test_gpu_export import MB_H, MB_W, SLOTS, STREAMS, TAIL
from tests.test_gpu_resize import SCALES

pytestmark = pytest.mark.gpu

BATCH_RING = 4                      # staging buffers of the ring (p264hip.hip)
ROI_WORDS = 8                       # a descriptor: 32 bytes (kernel_roi.h: RoiDev)
FRAME, MID, INSIDE, SMALL, CORNER = (0, 0, 80, 48), (2, 2, 62, 30), (18, 10, 34, 18), (16, 10, 8, 8), (6, 46, 2, 2)
PICS = [(s, k) for s in range(STREAMS) for k in range(SLOTS)]
# the 40 ROIs of the sixth call into a 10 x 6 output: every picture, four windows, the whole output and three rectangles
MANY = [PICS[i % 6] + (FRAME, MID, SMALL, CORNER)[i % 4] + ((), (2, 0, 8, 6), (0, 2, 10, 2), (4, 2, 2, 4))[(i // 4) % 4] for i in range(40)]

# (road, pictures or ROIs, output size, format, dtype, what else the call says): in the order they are queued
CALLS = [
    ("resized", [(2, 1)], (2, 2), "rgbp", "u8", dict(crop=CORNER)),
    ("resized_aa", [(0, 0), (1, 1)], (4, 4), "rgb24", "f16", dict(crop=SMALL, scale=SCALES[1][0], bias=SCALES[1][1], offset=2)),
    ("rois", [(0, 1) + FRAME, (2, 0) + MID + (2, 2, 30, 14), (1, 0) + CORNER + (32, 16, 2, 2)], (34, 18), "i420", "u8", dict(fill=(235, 16, 240))),
    ("rois_aa", [(1, 1) + MID + (6, 0, 22, 18), (0, 0) + FRAME], (34, 18), "rgbp", "f32", dict(scale=SCALES[0][0], bias=SCALES[0][1], matrix="bt709", full=True)),
    ("frames", [(2, 0), (0, 1), (2, 0)], INSIDE[2:], "nv12", "u8", dict(crop=INSIDE, offset=1, stride=34 * 18 * 3 // 2 + 7)),
    ("rois", MANY, (10, 6), "rgb24", "u8", dict(fill=(0, 255, 0), matrix="bt709")),
    ("resized", [(1, 0), (2, 1), (0, 0)], (34, 18), "i420", "u8", dict(crop=FRAME, pitch=50)),
    ("resized_aa", [(2, 1), (1, 0)], (34, 18), "nv12", "u8", dict(crop=FRAME, offset=4)),
    ("rois_aa", [(0, 1) + FRAME + (2, 2, 30, 14), (2, 0) + MID, (1, 1) + SMALL + (0, 4, 34, 2)], (34, 18), "rgb24", "f16", dict(scale=SCALES[1][0], bias=SCALES[1][1])),
]


def pad4(n):
    return (n + 3) & ~3


def table_words(road, items, size, crop):
    """words of the call's table, from its shapes (include/p264hip.h and the kernel headers describe the tables)"""
    n, (W, H) = len(items), size
    if road == "frames":
        return n                                                    # a frame index per picture
    if road in ("rois", "rois_aa"):
        return n * ROI_WORDS
    if road == "resized":                                           # the indices, then a word per destination sample of the four axes
        return pad4(n) + pad4(W) + pad4(H) + pad4(W // 2) + pad4(H // 2)
    words = pad4(n)                                                 # antialiased: a word and a row of 16-bit weights per destination sample
    for S, D in ((crop[2], W), (crop[3], H), (crop[2] // 2, W // 2), (crop[3] // 2, H // 2)):
        stride = (int(KA.taps(S, D)[1].max()) + 1) & ~1
        words += pad4(D) + pad4(D * stride // 2)
    return words


def ring_growth():
    """the calls at which the ring grows by its rule - a table above the capacity makes it n + n // 2 + 16 words -, and every table's words"""
    cap, grew, words = 0, [], []
    for i, (road, items, size, fmt, dtype, kw) in enumerate(CALLS):
        words.append(table_words(road, items, size, kw.get("crop")))
        if words[-1] > cap:
            cap = words[-1] + words[-1] // 2 + 16
            grew.append(i)
    return grew, words


def expected(planes, road, items, size, fmt, dtype, total, crop=None, fill=K.FILL, scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """the whole destination of a call as its road's checker has it"""
    if road == "frames":
        return X.expected([planes[p] for p in items], fmt, crop, matrix, full, pitch, stride, offset, total)
    if road in ("resized", "resized_aa"):
        model = R.expected if road == "resized" else A.expected_aa
        return model([planes[p] for p in items], fmt, crop, size, dtype, scale, bias, matrix, full, pitch, stride, offset, total)
    model = K.expected if road == "rois" else KA.expected
    return model(items, planes, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, offset, total)


def queue(hip, road, items, size, fmt, dtype, out, crop=None, fill=K.FILL, scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """the call itself, left in flight"""
    if road == "frames":
        hip.export_frames([s for s, _ in items], [k for _, k in items], fmt, crop, matrix, full, pitch, out=out, sync=False, frame_stride=stride)
    elif road in ("resized", "resized_aa"):
        hip.export_resized([s for s, _ in items], [k for _, k in items], size, fmt, dtype, crop, scale, bias, matrix, full, pitch, stride, out=out, sync=False,
                           filter="bilinear" if road == "resized" else "bilinear_aa")
    else:
        (hip.export_rois if road == "rois" else hip.export_rois_aa)(items, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, out=out, sync=False)


@pytest.fixture
def store(lib):
    """a FRESH context (the staging ring is empty) whose six frames hold random planes, and those planes as read_frame returns them"""
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        g = np.random.default_rng(2671)
        w, h = MB_W * 16, MB_H * 16
        for s, k in PICS:
            hip.write_frame(s, k, g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8))
        yield hip, {p: hip.read_frame(*p) for p in PICS}


def test_nine_calls_in_flight_over_every_road(store):
    hip, planes = store
    assert len(CALLS) == 2 * BATCH_RING + 1 and {c[0] for c in CALLS} == {"frames", "resized", "resized_aa", "rois", "rois_aa"}
    assert all(size[0] <= 34 and size[1] <= 18 and (1 <= len(items) <= 3 or i == 5) for i, (_, items, size, _, _, _) in enumerate(CALLS))
    # the first call sizes the ring, the next four fit it, the sixth alone exceeds it
    grew, words = ring_growth()
    assert words[0] == 20 and words[5] == 40 * ROI_WORDS and max(words[1:5]) <= 20 + 20 // 2 + 16 < words[5] and grew == [0, 5], (grew, words)
    # every destination before the first call (a DeviceBuffer's prefill waits for the device)
    dsts = []
    for road, items, size, fmt, dtype, kw in CALLS:
        per = X.frame_bytes(fmt, size[0], size[1], kw.get("pitch", 0)) if road == "frames" else R.frame_bytes(fmt, size[0], size[1], dtype, kw.get("pitch", 0))
        total = kw.get("offset", 0) + (len(items) - 1) * (kw.get("stride", 0) or per) + per + TAIL
        dsts.append((DeviceBuffer(hip.lib, total), total))
    for (road, items, size, fmt, dtype, kw), (dst, total) in zip(CALLS, dsts):
        offset = kw.get("offset", 0)
        queue(hip, road, items, size, fmt, dtype, (dst.ptr + offset, total - offset - TAIL), **kw)
    hip.sync()
    for i, ((road, items, size, fmt, dtype, kw), (dst, total)) in enumerate(zip(CALLS, dsts)):
        got, want = dst.host(), expected(planes, road, items, size, fmt, dtype, total, **kw)
        dst.free()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "call %d (%s, %d pictures to %s as %s %s, %s): %d of %d bytes differ, the first at %d (%d, want %d)" % (
            i + 1, road, len(items), size, fmt, dtype, kw, bad.size, total, bad[0], got[bad[0]], want[bad[0]])
