"""The pipeline's exit for per-picture windows from an ROI list in device memory (p264pipe_export_last_rois_device): between runs and
from inside the callback of a decode-order sink, both filters, equal to p264pipe_export_last_rois of the same rows; a stream without
a picture yet gives the status NO_PICTURE and an untouched picture.  The streams of tests/test_gpu_roi_pipeline.py: 8 x 6
macroblocks, unequal lengths."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import Pipeline, _native as N
from tests import resize_checker as R
from tests import roi_device_checker as DK
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export_pipeline import FRAMES, make_streams
from tests.test_gpu_roi_pipeline import NORM, SIZE, rows_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def streams():
    return make_streams((8, 6), FRAMES, "0 3 0 2", 70)


def device_rows(lib, rows):
    """the pipeline's rows (stream, window[, rectangle]) as p264hip_roi_t rows with slot -1, in device memory"""
    a = np.array([(r[0], -1) + tuple(r[1:]) + (0, 0, 0, 0) * (len(r) == 5) for r in rows], np.int32)
    buf = DeviceBuffer(lib, a.nbytes)
    assert lib.p264hip_copy_to_device(buf.ptr, a.ctypes.data, a.nbytes) == 0
    return buf


def both(pipe, lib, rows, fmt, dtype, filter, scale, bias, per, bufs):
    """the device-list call and the host-list call for the same rows: (bytes, status words, bytes of the host list)"""
    got, status, host = bufs
    for b in bufs:
        b.fill(0xA5)
    d = device_rows(lib, rows)
    pipe.export_last_rois_device((d.ptr, len(rows)), SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(got.ptr, len(rows) * per), status=status.ptr, filter=filter, stream=None)
    pipe.export_last_rois(rows, SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(host.ptr, len(rows) * per), filter=filter)
    d.free()
    return got.host(), status.host()[:4 * len(rows)].view(np.int32).tolist(), host.host()


@pytest.mark.parametrize("fmt,dtype,filter", [("nv12", "u8", "bilinear"), ("rgbp", "f32", "bilinear_aa")])
def test_between_runs_and_before_the_first(lib, streams, fmt, dtype, filter):
    n = len(streams)
    scale, bias = NORM if dtype != "u8" else (None, None)
    per = R.frame_bytes(fmt, SIZE[0], SIZE[1], dtype)
    rows, _ = rows_of([2, 0, 1, 2])
    bufs = [DeviceBuffer(lib, len(rows) * per + 16), DeviceBuffer(lib, 4 * len(rows) + 16), DeviceBuffer(lib, len(rows) * per + 16)]
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    d = device_rows(lib, rows)
    with pytest.raises(RuntimeError):                       # before the first run there is no device context
        pipe.export_last_rois_device((d.ptr, len(rows)), SIZE, fmt, dtype, scale=scale, bias=bias, out=(bufs[0].ptr, len(rows) * per), filter=filter, stream=None)
    pipe.run()
    got, status, host = both(pipe, lib, rows, fmt, dtype, filter, scale, bias, per, bufs)
    assert status == [0] * len(rows)
    assert np.array_equal(got, host) and not np.all(got[:per] == 0xA5)
    # the caller's slot table is refused; a stream that does not exist and a window that leaves the frame are statuses, not refusals
    r = N.resize_desc(fmt, SIZE, (0, 0, 2, 2), None, dtype, scale, bias, filter=filter)
    l = N.RoisDev(d.ptr, None, None, (C.c_int32 * n)(), None, None, len(rows), 0, 0)
    assert lib.p264pipe_export_last_rois_device(pipe.h, C.byref(l), C.byref(r), 0, bufs[0].ptr, len(rows) * per) == -1
    d.free()
    bad = [(n,) + rows[0][1:], rows[1], (1, 64, 2, 24, 96)]
    d = device_rows(lib, bad)
    for b in bufs:
        b.fill(0xA5)
    pipe.export_last_rois_device((d.ptr, 3), SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(bufs[0].ptr, 3 * per), status=bufs[1].ptr, filter=filter, stream=None)
    assert bufs[1].host()[:12].view(np.int32).tolist() == [DK.BAD_PICTURE, 0, DK.WINDOW_OUTSIDE]
    after = bufs[0].host()
    assert np.all(after[:per] == 0xA5) and np.array_equal(after[per:2 * per], host[per:2 * per]) and np.all(after[2 * per:] == 0xA5)
    pipe.close()
    for b in bufs + [d]:
        b.free()


def header_only(lib, data):
    """the stream up to its first slice: parameter sets and no picture"""
    for nal_type, _, _ in N.split_annexb(lib, data):
        assert nal_type in (1, 5, 6, 7, 8, 9)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    pos, off, ln = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    while lib.p264_annexb_next(buf, len(data), C.byref(pos), C.byref(off), C.byref(ln)):
        if ln.value > 0 and data[off.value] & 0x1F in (1, 5):
            return data[:off.value - 3]
    raise AssertionError("no slice in the stream")


@pytest.mark.parametrize("filter", ["bilinear", "bilinear_aa"])
def test_from_inside_a_decode_order_sink(lib, streams, filter):
    """a fourth stream never has a picture.  Every round's callback asks for two windows of EVERY stream: those of the three streams
    are export_last_rois' of the same rows - the round's pictures, or the last one of a stream that has ended -, those of the
    fourth are NO_PICTURE and stay untouched"""
    n = len(streams) + 1
    per = R.frame_bytes("rgbp", SIZE[0], SIZE[1], "f16")
    rows, _ = rows_of(list(range(n)))
    room = [DeviceBuffer(lib, 1 << 20) for _ in range(2)]
    bufs = [DeviceBuffer(lib, len(rows) * per + 16), DeviceBuffer(lib, 4 * len(rows) + 16), DeviceBuffer(lib, len(rows) * per + 16)]
    pipe = Pipeline(list(streams) + [header_only(lib, streams[0])], threads=n, device=0, lib=lib)
    rounds = []

    def sink(rnd, which, dev, nbytes):
        for b in bufs:
            b.fill(0xA5)
        d = device_rows(lib, rows)
        pipe.export_last_rois_device((d.ptr, len(rows)), SIZE, "rgbp", "f16", (235, 16, 240), NORM[0], NORM[1], out=(bufs[0].ptr, len(rows) * per), status=bufs[1].ptr, filter=filter,
                                     stream=None)
        pipe.export_last_rois(rows[:-2], SIZE, "rgbp", "f16", (235, 16, 240), NORM[0], NORM[1], out=(bufs[2].ptr, (len(rows) - 2) * per), filter=filter)
        d.free()
        rounds.append((rnd, list(which), bufs[0].host(), bufs[1].host()[:4 * len(rows)].view(np.int32).tolist(), bufs[2].host()))
    pipe.set_sink("i420", sink, buffers=[(b.ptr, b.nbytes) for b in room])
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and [r[0] for r in rounds] == list(range(max(FRAMES)))
    assert all(n - 1 not in r[1] for r in rounds) and rows[-1][0] == rows[-2][0] == n - 1
    for rnd, which, got, status, host in rounds:
        k = len(rows) - 2
        assert status == [0] * k + [DK.NO_PICTURE] * 2, "round %d" % rnd
        assert np.array_equal(got[:k * per], host[:k * per]) and not np.all(host[:per] == 0xA5), "round %d" % rnd
        assert np.all(got[k * per:] == 0xA5), "round %d: a picture of the stream without one was written" % rnd
    assert any(not np.array_equal(a[2][:per], b[2][:per]) for a, b in zip(rounds, rounds[1:]))        # (the rounds' pictures differ)
    pipe.close()
    for b in room + bufs:
        b.free()
