"""p264hip_export_rois_aa on the MI355X: a window per picture, each resized by the ANTIALIASED filter into a rectangle of the output
with a constant round it, in one call (include/p264hip.h; csrc/hip/kernel_roi_aa.h).  The fixture is tests/test_gpu_roi.py's: 5 x 3
macroblocks, 3 streams x 2 slots of random planes.  Every test prefills the whole destination with 0xA5 and compares ALL of it,
floats as bytes, with tests/roi_aa_checker.py applied to the read_frame planes: a byte written outside the layout fails it.
Bit-exact, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from p264decoder_amd.recon import P264Error
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export import STREAMS, TAIL
from tests.test_gpu_resize import INSTANCES, WINDOWS
from tests.test_gpu_resize_aa import run as run_resized_aa
from tests.test_gpu_roi import FILLS, PICS, rotation, same, store  # noqa: F401  (store: the fixture)

pytestmark = pytest.mark.gpu

AA = N.FILTER_BILINEAR_AA
# output -> the ROIs of the mixed call: an enlargement, D == S, 2:1, an odd ratio, (0, 0, 64, 32) into 2 x 2 at the far corner (32:1 and
# 16:1), a window of 2 x 2, and picture (2, 1) a second time
MIXED = {
    (162, 98): [(0, 0, 16, 10, 48, 22, 2, 2, 96, 44), (2, 1, 16, 10, 48, 22, 100, 50, 48, 22), (1, 0, 0, 0, 80, 48, 4, 60, 40, 24), (0, 1, 2, 2, 62, 30, 60, 2, 22, 14),
                (1, 1, 0, 0, 64, 32, 160, 96, 2, 2), (2, 0, 78, 46, 2, 2, 120, 4, 6, 10), (2, 1, 0, 0, 80, 48, 0, 0, 0, 0)],
    (34, 18): [(0, 0, 6, 46, 8, 2, 0, 0, 20, 8), (2, 1, 16, 10, 20, 10, 12, 0, 20, 10), (1, 0, 0, 0, 40, 16, 0, 10, 20, 8), (0, 1, 2, 2, 62, 30, 22, 10, 10, 6),
               (1, 1, 0, 0, 64, 32, 32, 16, 2, 2), (2, 0, 78, 46, 2, 2, 30, 0, 2, 2), (2, 1, 2, 2, 62, 30)],
}


def run(hip, planes, rois, size, fmt, dtype="u8", fill=K.FILL, scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """one call into a prefilled destination; returns (what the device holds, what the checker says it holds)"""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    total = offset + (len(rois) - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_rois_aa(rois, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, out=(dst.ptr + offset, total - offset - TAIL))
    want = KA.expected(rois, planes, size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, offset, total, tag="store")
    got = dst.host()
    dst.free()
    return got, want


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_whole_rectangles_of_one_window_are_export_resized_aa(store, fmt, dtype):
    hip, planes = store
    n = 0
    for size in ((34, 18), (162, 98)):
        for window in (WINDOWS[1], WINDOWS[0]):
            kw = rotation(fmt, dtype, size, n)
            n += 1
            streams, slots = [2, 0, 1], [1, 0, 1]
            rois = [(s, k) + window + ((0, 0) + size if i == 1 else ()) for i, (s, k) in enumerate(zip(streams, slots))]
            got, want = run(hip, planes, rois, size, fmt, dtype, FILLS[n % 3], **kw)
            resized, model = run_resized_aa(hip, planes, streams, slots, fmt, window, size, dtype, kw["scale"], kw["bias"], kw["matrix"], kw["full"], kw["pitch"], kw["stride"], kw["offset"])
            same(resized, model, "export_resized %s %s %s to %s" % (fmt, dtype, window, size))
            same(got, resized, "%s %s %s to %s against export_resized %s" % (fmt, dtype, window, size, kw))
            same(got, want, "%s %s %s to %s against the model" % (fmt, dtype, window, size))


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_mixed_windows_in_one_call(store, fmt, dtype):
    hip, planes = store
    for n, (size, rois) in enumerate(MIXED.items()):
        assert len(rois) == 7 and len({r[:2] for r in rois}) < len(rois)
        kinds = [(r[4] / (r[8] if len(r) == 10 and r[8] else size[0]), r[5] / (r[9] if len(r) == 10 and r[9] else size[1])) for r in rois]
        assert kinds[0][0] < 1 and kinds[1] == (1, 1) and kinds[2] == (2, 2) and kinds[4] == (32, 16) and rois[5][4:6] == (2, 2) and kinds[3][0] not in (1, 2, 3, 4)
        kw = rotation(fmt, dtype, size, n + INSTANCES.index((fmt, dtype)))
        shift = INSTANCES.index((fmt, dtype)) % 7
        got, want = run(hip, planes, rois[shift:] + rois[:shift], size, fmt, dtype, FILLS[n], **kw)
        same(got, want, "%s %s to %s, %s" % (fmt, dtype, size, kw))


# output -> the rectangles of one call (None: the whole output); every one holds a reduction of the whole 80 x 48 frame unless it is 2 high
RECTANGLES = {
    (162, 98): [(58, 10, 20, 12), None, (10, 6, 140, 70)],          # the first crosses the tile column border at 64 and the row border at 16
    (34, 18): [None, (2, 2, 30, 14), (6, 0, 22, 18), (32, 16, 2, 2), (0, 4, 34, 2)],
    (518, 4): [None, (254, 0, 10, 4)],
}


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_rectangles_that_cross_tile_borders(store, fmt, dtype):
    hip, planes = store
    n = INSTANCES.index((fmt, dtype))
    for size, rects in RECTANGLES.items():
        for fill in FILLS if size == (34, 18) else [FILLS[n % 3]]:
            kw = rotation(fmt, dtype, size, n)
            n += 1
            rois = []
            for i, rect in enumerate(rects):
                dw, dh = rect[2:] if rect else size
                window = (0, 0, min(80, 32 * dw), min(48, 32 * dh))         # the whole frame, or what 32:1 lets in
                rois.append(PICS[(i + n) % 6] + window + (rect if rect else (0, 0, 0, 0)))
            rois += [PICS[(n + 3) % 6] + (16, 10) + rect[2:] + rect for rect in rects if rect and rect[2] <= 64 and rect[3] <= 38]      # ... and pasted: D == S
            got, want = run(hip, planes, rois, size, fmt, dtype, fill, **kw)
            same(got, want, "%s %s to %s fill %s, %s" % (fmt, dtype, size, fill, kw))


def test_more_rois_than_a_grid_dimension(store):
    """65 537 ROIs to 2 x 2 I420 (6 bytes each): both launches are split at 65 535 - and, their segments being 40 MB, at the scratch
    cap; the windows and pictures cycle through 96 combinations"""
    hip, planes = store
    windows = [(2 * (i % 5), 2 * (i // 5), 2 + 18 * (i % 4), 2 + 10 * (i // 4)) for i in range(16)]
    combos = [p + w for p in PICS for w in windows]
    assert len(combos) == 96 and all(w[0] + w[2] <= 80 and w[1] + w[3] <= 48 and w[2] <= 64 and w[3] <= 64 for w in windows)
    n = 65537
    which = (np.arange(n) * 7 + np.arange(n) // 65535) % 96                # (the pattern shifts at the seam)
    rois = np.array(combos, np.int32)[which]
    dst = DeviceBuffer(hip.lib, n * 6 + TAIL)
    hip.export_rois_aa(rois, (2, 2), "i420", out=(dst.ptr, n * 6))
    got = dst.host()
    dst.free()
    assert got.size == 393222 + TAIL
    table = np.stack([KA.expected([c], planes, (2, 2), "i420") for c in combos])
    assert np.array_equal(got[:n * 6].reshape(n, 6), table[which])
    assert np.all(got[n * 6:] == 0xA5)


def test_the_scratch_bound_crossed_by_one_roi(store):
    """outputs of 16384 x 2: the ROIs' segments (p264hip_roi_aa_segment_words) fill the scratch but for the last one, which goes out in
    a second pair of launches over segment 0; then a smaller call on the same context"""
    hip, planes = store
    lib = hip.lib
    size = (16384, 2)
    r = N.resize_desc("i420", size, (0, 0, 2, 2), None, filter=AA)
    combos = [PICS[i % 6] + w for i, w in enumerate(WINDOWS + [(0, 0, 2, 2), (78, 46, 2, 2), (0, 0, 80, 2)])]
    words = [lib.p264hip_roi_aa_segment_words(C.byref(N.Roi(*c, 0, 0, 0, 0)), C.byref(r)) for c in combos]
    assert min(words) > 16384 + 8192
    cap = N.ROI_SCRATCH_BYTES // 4
    n, used = 0, 0
    while used <= cap:
        used += words[n % 7]
        n += 1
    assert used > cap >= used - words[(n - 1) % 7] and 60 < n < 200           # ROI n - 1 is the one that no longer fits
    which = np.arange(n) % 7
    assert which[n - 1] != which[0]                                         # (the ROI that reuses segment 0 is not the one that had it)
    per = R.frame_bytes("i420", *size)
    dst = DeviceBuffer(lib, n * per + TAIL)
    hip.export_rois_aa([combos[w] for w in which], size, "i420", fill=(1, 2, 3), out=(dst.ptr, n * per))
    got = dst.host()
    dst.free()
    table = np.stack([KA.expected([c], planes, size, "i420", fill=(1, 2, 3)) for c in combos])
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
        return lib.p264hip_export_rois_aa(ctx, arr, len(rois) if n is None else n, C.byref(r) if r is not None else None, fill, d, cap)

    def D(fmt="rgbp", size=size, dtype="f16", scale=1 / 255, filter=AA, **kw):
        return N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, filter=filter, **kw)

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
        lambda: call(D(filter=0)), lambda: call(D(filter=1)), lambda: call(D(filter=-1)), lambda: call(D(), fill=word | 1 << 24),
        # beyond 32:1 (in width: this frame is 48 high, and 48 into 2 is 24:1 - tests/test_roi_aa_cpu.py has the height)
        lambda: call(D(), rois=second(left=0, width=66, dst_width=2)), lambda: call(D(), rois=second(left=0, top=0, width=80, height=48, dst_width=2, dst_height=2)),
        lambda: call(D(size=(2, 2)), rois=[N.Roi(0, 0, 0, 0, 66, 2, 0, 0, 0, 0)], cap=2 * per),
        lambda: call(D(fmt=4)), lambda: call(D(matrix=2)), lambda: call(D("i420")), lambda: call(D(dtype=3)),
        lambda: call(D(dtype="u8")), lambda: call(D(scale=float("nan"))), lambda: call(D(size=(33, 18))), lambda: call(D(size=(16386, 2))),
        lambda: call(D(pitch=66)), lambda: call(D(pitch=71)), lambda: call(D(frame_stride=per - 2)), lambda: call(D(frame_stride=per + 1)),
        lambda: call(D(), cap=2 * per - 1), lambda: call(D(frame_stride=per + 8), cap=2 * per + 7), lambda: call(D(), d=ptr + 1, cap=2 * per),
    ]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_rois_aa:"), (i, lib.p264hip_last_error())
    assert call(D(), rois=second(dst_left=14)) == -1 and b"ROI 1:" in lib.p264hip_last_error()          # the message names the first bad ROI
    assert call(D(), rois=second(left=0, width=66, dst_width=2)) == -1 and b"ROI 1:" in lib.p264hip_last_error() and b"32:1" in lib.p264hip_last_error()
    assert call(D(), rois=[N.Roi(0, 0, 0, 0, 80, 48, 4, 4, 2, 2)] + good) == -1 and b"ROI 0:" in lib.p264hip_last_error()
    hip.sync()
    assert np.all(dst.host() == 0xA5)
    with pytest.raises(P264Error):
        hip.export_rois_aa([(0, 0, 2, 2, 62, 30), (STREAMS, 0, 2, 2, 62, 30)], size, out=(ptr, total))
    with pytest.raises(P264Error):
        hip.export_rois_aa([(0, 0, 2, 2, 62, 30)], size, "nv12", "f32", out=(ptr, total))
    with pytest.raises(P264Error):
        hip.export_rois_aa([(0, 0, 0, 0, 80, 48, 0, 0, 2, 2)], size, "rgbp", "f16", scale=1 / 255, out=(ptr, total))
    assert np.all(dst.host() == 0xA5)
    # any crop_* in the description: not read
    r = D()
    r.crop_left, r.crop_top, r.crop_width, r.crop_height = 1, -3, 0, 1 << 30
    assert call(r) == 0
    hip.sync()
    rows = [(0, 0, 2, 2, 62, 30), (1, 1, 16, 10, 48, 22, 6, 0, 22, 18)]
    assert np.array_equal(dst.host(), KA.expected(rows, planes, size, "rgbp", "f16", K.FILL, 1 / 255, None, total=total))
    dst.free()


def test_the_filter_0_entry_still_refuses_filter_2(store):
    """... beside the new entry accepting it, and the new entry refusing filter 0 beside the old one accepting it"""
    hip, planes = store
    lib = hip.lib
    size = (34, 18)
    per = R.frame_bytes("nv12", *size)
    rows = [(0, 0, 2, 2, 62, 30), (1, 1, 16, 10, 48, 22, 6, 0, 22, 18)]
    arr, n = N.roi_array(rows)
    word = N.fill_word(K.FILL)
    dst = DeviceBuffer(lib, 2 * per + TAIL)
    for filt, old, new in ((AA, -1, 0), (0, 0, -1)):
        r = N.resize_desc("nv12", size, (0, 0, 2, 2), None, filter=filt)
        for entry, rc, model in ((lib.p264hip_export_rois, old, K), (lib.p264hip_export_rois_aa, new, KA)):
            dst.fill(0xA5)
            assert entry(hip.h, arr, n, C.byref(r), word, dst.ptr, 2 * per) == rc, (filt, entry)
            hip.sync()
            want = model.expected(rows, planes, size, "nv12", total=2 * per + TAIL) if rc == 0 else np.full(2 * per + TAIL, 0xA5, np.uint8)
            same(dst.host(), want, "filter %d" % filt)
        assert lib.p264hip_rois_frame_bytes(C.byref(r)) == (per if filt == 0 else -1) and lib.p264hip_rois_aa_frame_bytes(C.byref(r)) == (per if filt == AA else -1)
    with pytest.raises(P264Error):
        hip._export_rois(rows, size, "nv12", "u8", K.FILL, None, None, "bt601", False, 0, 0, (dst.ptr, 2 * per), True, 1)     # filter 1: not assigned
    dst.free()
