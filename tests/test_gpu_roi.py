"""p264hip_export_rois on the MI355X: a window per picture, each resized into a rectangle of the output with a constant round it, in
one call (include/p264hip.h: p264hip_roi_t; csrc/hip/kernel_roi.h).  The fixture is tests/test_gpu_resize.py's: 5 x 3 macroblocks,
3 streams x 2 slots of random planes.  Every test prefills the whole destination with 0xA5 and compares ALL of it, floats as bytes,
with tests/roi_checker.py applied to the read_frame planes: a byte written outside the layout fails it.  Bit-exact, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from p264decoder_amd.recon import P264Error
from tests import resize_checker as R
from tests import roi_checker as K
from tests.device_mem import DeviceBuffer
from tests.hip_harness import reconstructor
from tests.test_gpu_resize import ELEM, INSTANCES, RGB_KINDS, SCALES, WINDOWS, run as run_resized
from tests.test_gpu_export import MB_H, MB_W, SLOTS, STREAMS, TAIL

pytestmark = pytest.mark.gpu

FILLS = [(16, 128, 128), (235, 16, 240), (0, 255, 0)]      # (the last one so that RGB clips)
# the seven ROIs of the mixed call: the four windows, the two corner windows of 2 x 2 samples, and picture (2, 1) a second time
MIXED = [(0, 0) + WINDOWS[0], (2, 1) + WINDOWS[1], (1, 0) + WINDOWS[2], (0, 1) + WINDOWS[3], (1, 1, 0, 0, 2, 2), (2, 0, 78, 46, 2, 2), (2, 1) + WINDOWS[2]]
PICS = [(s, k) for s in range(STREAMS) for k in range(SLOTS)]


@pytest.fixture(scope="module")
def store(lib):
    """a context whose six frames hold random planes, and those planes as read_frame returns them"""
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        g = np.random.default_rng(2662)
        w, h = MB_W * 16, MB_H * 16
        for s, k in PICS:
            hip.write_frame(s, k, g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8))
        yield hip, {p: hip.read_frame(*p) for p in PICS}


def run(hip, planes, rois, size, fmt, dtype="u8", fill=K.FILL, scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """one call into a prefilled destination; returns (what the device holds, what the checker says it holds)"""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    total = offset + (len(rois) - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_rois(rois, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, out=(dst.ptr + offset, total - offset - TAIL))
    want = K.expected(rois, planes, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, offset, total, tag="store")
    got = dst.host()
    dst.free()
    return got, want


def rotation(fmt, dtype, size, n):
    """the n-th choice of pitch, destination offset, frame stride, matrix / range and scale set (tests/test_gpu_resize.py's sweep)"""
    elem = ELEM[dtype]
    tight = R.tight_pitch(fmt, size[0], dtype)
    pitch = (0, tight + 16, tight + 2 * elem)[n % 3]
    if fmt == "i420" and pitch % 2:
        pitch += 1
    offset = (0, elem, 4)[(n // 3) % 3]
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    stride = 0 if (n // 2) % 2 == 0 else per + 8
    matrix, full = RGB_KINDS[n % 4] if fmt.startswith("rgb") else ("bt601", False)
    scale, bias = SCALES[(n // 4) % 2] if dtype != "u8" else (None, None)
    return dict(scale=scale, bias=bias, matrix=matrix, full=full, pitch=pitch, stride=stride, offset=offset)


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d (%d, want %d)" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_whole_rectangles_of_one_window_are_export_resized(store, fmt, dtype):
    hip, planes = store
    n = 0
    for size in ((34, 18), (162, 98)):
        for window in (WINDOWS[1], WINDOWS[0]):
            kw = rotation(fmt, dtype, size, n)
            n += 1
            streams, slots = [2, 0, 1], [1, 0, 1]
            rois = [(s, k) + window + ((0, 0) + size if i == 1 else ()) for i, (s, k) in enumerate(zip(streams, slots))]
            got, want = run(hip, planes, rois, size, fmt, dtype, FILLS[n % 3], **kw)
            resized, model = run_resized(hip, planes, streams, slots, fmt, window, size, dtype, kw["scale"], kw["bias"], kw["matrix"], kw["full"], kw["pitch"], kw["stride"], kw["offset"])
            same(resized, model, "export_resized %s %s %s to %s" % (fmt, dtype, window, size))
            same(got, resized, "%s %s %s to %s against export_resized %s" % (fmt, dtype, window, size, kw))
            same(got, want, "%s %s %s to %s against the model" % (fmt, dtype, window, size))


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_mixed_windows_in_one_call(store, fmt, dtype):
    hip, planes = store
    assert len(MIXED) >= 7 and len({r[:2] for r in MIXED}) < len(MIXED)
    for n, size in enumerate(((34, 18), (162, 98), (6, 70), (2, 2), (34, 18), (162, 98), (6, 70), (2, 2))):
        kw = rotation(fmt, dtype, size, n + INSTANCES.index((fmt, dtype)))
        rois = MIXED[n % 7:] + MIXED[:n % 7]
        got, want = run(hip, planes, rois, size, fmt, dtype, **kw)
        same(got, want, "%s %s to %s, %s" % (fmt, dtype, size, kw))


# output -> the rectangles of one call (None: the whole output)
RECTANGLES = {
    (34, 18): [None, (2, 2, 30, 14), (6, 0, 22, 18), (32, 16, 2, 2), (0, 0, 2, 2), (0, 4, 34, 2)],
    (162, 98): [(10, 6, 140, 70), None],
    (518, 4): [None, (254, 0, 10, 4)],
}


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_rectangles_mixed_in_one_call(store, fmt, dtype):
    hip, planes = store
    n = INSTANCES.index((fmt, dtype))
    for size, rects in RECTANGLES.items():
        for fill in FILLS if size == (34, 18) else [FILLS[n % 3]]:
            kw = rotation(fmt, dtype, size, n)
            n += 1
            rois = [MIXED[(i + n) % 7] + (rect if rect else (0, 0, 0, 0)) for i, rect in enumerate(rects)]
            rois += [MIXED[(n + 3) % 7][:2] + (16, 10) + rect[2:] + rect for rect in rects if rect and rect[2] <= 64 and rect[3] <= 38]      # ... and pasted: D == S
            got, want = run(hip, planes, rois, size, fmt, dtype, fill, **kw)
            same(got, want, "%s %s to %s fill %s, %s" % (fmt, dtype, size, fill, kw))


def test_more_rois_than_a_grid_dimension(store):
    """65 537 ROIs to 2 x 2 I420 (6 bytes each): both launches are split at 65 535; the windows and pictures cycle through 96 combinations"""
    hip, planes = store
    windows = [(2 * (i % 5), 2 * (i // 5), 2 + 18 * (i % 4), 2 + 10 * (i // 4)) for i in range(16)]
    combos = [p + w for p in PICS for w in windows]
    assert len(combos) == 96 and all(w[0] + w[2] <= 80 and w[1] + w[3] <= 48 for w in windows)
    n = 65537
    which = (np.arange(n) * 7 + np.arange(n) // 65535) % 96                # (the pattern shifts at the seam)
    rois = np.array(combos, np.int32)[which]
    dst = DeviceBuffer(hip.lib, n * 6 + TAIL)
    hip.export_rois(rois, (2, 2), "i420", out=(dst.ptr, n * 6))
    got = dst.host()
    dst.free()
    assert got.size == 393222 + TAIL
    table = np.stack([K.expected([c], planes, (2, 2), "i420") for c in combos])
    assert np.array_equal(got[:n * 6].reshape(n, 6), table[which])
    assert np.all(got[n * 6:] == 0xA5)


def test_the_scratch_bound_crossed(store):
    """outputs of 16384 x 2: a segment is 24 584 words, so the 171st ROI no longer fits the scratch and goes out in a second pair of launches"""
    hip, planes = store
    size = (16384, 2)
    words = 16384 + 4 + 8192 + 4
    n = (N.ROI_SCRATCH_BYTES // 4) // words + 1
    assert n * words * 4 > N.ROI_SCRATCH_BYTES >= (n - 1) * words * 4 and n == 171
    combos = [PICS[i % 6] + w for i, w in enumerate(WINDOWS + [(0, 0, 2, 2), (78, 46, 2, 2), (0, 0, 80, 2)])]
    which = np.arange(n) % 7
    assert which[n - 1] != which[0]                                         # (the ROI that reuses segment 0 is not the one that had it)
    per = R.frame_bytes("i420", *size)
    dst = DeviceBuffer(hip.lib, n * per + TAIL)
    hip.export_rois([combos[w] for w in which], size, "i420", fill=(1, 2, 3), out=(dst.ptr, n * per))
    got = dst.host()
    dst.free()
    table = np.stack([K.expected([c], planes, size, "i420", fill=(1, 2, 3)) for c in combos])
    assert np.array_equal(got[:n * per].reshape(n, per), table[which])
    assert np.all(got[n * per:] == 0xA5)
    # the same ROIs, a rectangle each, in a call that fits: the scratch is reused by a smaller call behind a larger one
    rois = [c + (4 * i, 0, 16384 - 8 * i, 2) for i, c in enumerate(combos)]
    got, want = run(hip, planes, rois, size, "nv12", fill=(9, 8, 7))
    same(got, want, "16384 x 2 with rectangles")


def test_refusals_queue_nothing(store):
    hip, planes = store
    lib = hip.lib
    size = (34, 18)
    per = R.frame_bytes("rgbp", 34, 18, "f16")
    total = 2 * per + TAIL
    dst = DeviceBuffer(lib, total)
    ptr = dst.ptr
    good = [N.Roi(0, 0, 2, 2, 62, 30, 0, 0, 0, 0), N.Roi(1, 1, 16, 10, 48, 22, 6, 0, 22, 18)]
    word = N.fill_word((16, 128, 128))

    def call(r, rois=good, n=None, fill=word, d=ptr, cap=2 * per, ctx=hip.h):
        arr = (N.Roi * len(rois))(*rois) if rois is not None else None
        return lib.p264hip_export_rois(ctx, arr, len(rois) if n is None else n, C.byref(r) if r is not None else None, fill, d, cap)

    def D(fmt="rgbp", size=size, dtype="f16", scale=1 / 255, **kw):
        return N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, **kw)

    def second(**kw):
        f = dict(stream=1, slot=1, left=16, top=10, width=48, height=22, dst_left=6, dst_top=0, dst_width=22, dst_height=18)
        f.update(kw)
        return [good[0], N.Roi(*[f[k] for k, _ in N.Roi._fields_])]
    assert call(D()) == 0
    hip.sync()
    dst.fill(0xA5)
    refused = [
        lambda: call(D(), ctx=None), lambda: call(D(), rois=None, n=2), lambda: call(None), lambda: call(D(), d=None), lambda: call(D(), n=0),
        lambda: call(D(), rois=second(stream=STREAMS)), lambda: call(D(), rois=second(slot=-1)),
        lambda: call(D(), rois=second(left=15)), lambda: call(D(), rois=second(width=0)), lambda: call(D(), rois=second(left=34)), lambda: call(D(), rois=second(top=28)),
        lambda: call(D(), rois=second(dst_left=5)), lambda: call(D(), rois=second(dst_left=14)), lambda: call(D(), rois=second(dst_height=20)),
        lambda: call(D(), rois=second(dst_left=0, dst_top=0, dst_width=0, dst_height=2)), lambda: call(D(), rois=second(dst_left=0, dst_top=0, dst_width=34, dst_height=0)),
        lambda: call(D(filter=2)), lambda: call(D(filter=1)), lambda: call(D(), fill=word | 1 << 24),
        lambda: call(D(fmt=4)), lambda: call(D(matrix=2)), lambda: call(D("i420")), lambda: call(D(dtype=3)),
        lambda: call(D(dtype="u8")), lambda: call(D(scale=float("nan"))), lambda: call(D(size=(33, 18))), lambda: call(D(size=(16386, 2))),
        lambda: call(D(pitch=66)), lambda: call(D(pitch=71)), lambda: call(D(frame_stride=per - 2)), lambda: call(D(frame_stride=per + 1)),
        lambda: call(D(), cap=2 * per - 1), lambda: call(D(frame_stride=per + 8), cap=2 * per + 7), lambda: call(D(), d=ptr + 1, cap=2 * per),
    ]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_rois:"), i
    assert call(D(), rois=second(dst_left=14)) == -1 and b"ROI 1:" in lib.p264hip_last_error()          # the message names the first bad ROI
    hip.sync()
    assert np.all(dst.host() == 0xA5)
    with pytest.raises(P264Error):
        hip.export_rois([(0, 0, 2, 2, 62, 30), (STREAMS, 0, 2, 2, 62, 30)], size, out=(ptr, total))
    with pytest.raises(P264Error):
        hip.export_rois([(0, 0, 2, 2, 62, 30)], size, "nv12", "f32", out=(ptr, total))
    assert np.all(dst.host() == 0xA5)
    # any crop_* in the description: not read
    r = D()
    r.crop_left, r.crop_top, r.crop_width, r.crop_height = 1, -3, 0, 1 << 30
    assert call(r) == 0
    hip.sync()
    rows = [(0, 0, 2, 2, 62, 30), (1, 1, 16, 10, 48, 22, 6, 0, 22, 18)]
    assert np.array_equal(dst.host(), K.expected(rows, planes, size, "rgbp", "f16", K.FILL, 1 / 255, None, total=total))
    dst.free()
