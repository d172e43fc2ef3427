"""The pipeline's exit for per-picture windows (p264pipe_export_last_rois): windows of the streams' last decoded pictures, each resized
into a rectangle of the output - after a run, and from inside the callback of a decode-order sink, where the round's pictures are
the last decoded ones (the detect-then-crop cascade).  The streams of tests/test_gpu_resize_pipeline.py: 8 x 6 macroblocks, unequal
lengths; every crop must be tests/roi_checker.py's on the pictures each stream gives when it is decoded alone."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline, letterbox
from tests import export_checker as X
from tests import resize_checker as R
from tests import roi_checker as K
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export_pipeline import FRAMES, WINDOW, decode_alone, make_streams

pytestmark = pytest.mark.gpu

SIZE = (50, 38)
NORM = ([1 / (255 * s) for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])
# two windows of a picture: one over the whole output, one letterboxed
WIDE, TALL = (10, 20, 100, 30), (64, 2, 24, 90)


@pytest.fixture(scope="module")
def streams():
    return make_streams((8, 6), FRAMES, "0 3 0 2", 70)


@pytest.fixture(scope="module")
def alone(lib, streams):
    return decode_alone(lib, streams, (8, 6), FRAMES, WINDOW)


def rows_of(which):
    """the pipeline's rows for the streams `which`, and the model's (slot 0 stands for the stream's picture)"""
    rows = []
    for s in which:
        rows += [(s,) + WIDE, (s,) + TALL + letterbox(TALL[2], TALL[3], *SIZE)]
    return rows, [(r[0], 0) + r[1:] for r in rows]


@pytest.mark.parametrize("fmt,dtype", [("nv12", "u8"), ("rgbp", "f32"), ("rgb24", "f16")])
def test_export_last_rois_after_a_run(lib, streams, alone, fmt, dtype):
    n = len(streams)
    scale, bias = NORM if dtype != "u8" else (None, None)
    assert letterbox(TALL[2], TALL[3], *SIZE) == (20, 0, 10, 38)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    per = R.frame_bytes(fmt, SIZE[0], SIZE[1], dtype)
    rows, model = rows_of([2, 0, 1, 2])
    out = DeviceBuffer(lib, len(rows) * per + 16)
    with pytest.raises(RuntimeError):                                       # before the first run no stream has a picture
        pipe.export_last_rois(rows, SIZE, fmt, dtype, scale=scale, bias=bias, out=(out.ptr, len(rows) * per))
    pipe.run()
    pipe.export_last_rois(rows, SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(out.ptr, len(rows) * per))
    last = {(s, 0): alone[s][-1] for s in range(n)}
    assert np.array_equal(out.host(), K.expected(model, last, SIZE, fmt, dtype, (235, 16, 240), scale, bias, total=len(rows) * per + 16))
    # a stream that does not exist, a window that leaves the frame: refused, nothing written
    out.fill(0xA5)
    for bad in ([(n,) + WIDE], [(0,) + WIDE, (1, 64, 2, 24, 96)]):
        with pytest.raises(RuntimeError):
            pipe.export_last_rois(bad, SIZE, fmt, dtype, scale=scale, bias=bias, out=(out.ptr, len(rows) * per))
    assert np.all(out.host() == 0xA5)
    pipe.close()
    out.free()


def test_crops_from_inside_a_decode_order_sink(lib, streams, alone):
    """an I420 sink whose callback asks for two windows of every picture of the round: every round's crops are the model's on that
    round's pictures, and the sink's own buffers are what they are without the extra call"""
    n = len(streams)
    per_sink = X.frame_bytes("i420", WINDOW[2], WINDOW[3])
    per = R.frame_bytes("rgbp", SIZE[0], SIZE[1], "f16")
    room = [DeviceBuffer(lib, n * per_sink) for _ in range(2)]
    crops = DeviceBuffer(lib, 2 * n * per + 16)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    rounds = []

    def sink(rnd, which, dev, nbytes):
        rows, model = rows_of(which)
        crops.fill(0xA5)
        pipe.export_last_rois(rows, SIZE, "rgbp", "f16", scale=NORM[0], bias=NORM[1], out=(crops.ptr, len(rows) * per))
        host = np.empty(len(which) * nbytes, np.uint8)
        assert lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        rounds.append((rnd, list(which), host, crops.host(), model))
    assert pipe.set_sink("i420", sink, buffers=[(b.ptr, b.nbytes) for b in room]) == per_sink
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and [r[0] for r in rounds] == list(range(max(FRAMES)))
    assert [r[1] for r in rounds] == [[s for s in range(n) if FRAMES[s] > rnd] for rnd in range(max(FRAMES))]
    for rnd, which, host, got, model in rounds:
        assert np.array_equal(host, X.expected([alone[s][rnd] for s in which], "i420", WINDOW)), "the sink's buffer of round %d" % rnd
        now = {(s, 0): alone[s][rnd] for s in which}
        want = K.expected(model, now, SIZE, "rgbp", "f16", K.FILL, NORM[0], NORM[1], total=2 * n * per + 16)
        assert np.array_equal(got, want), "the crops of round %d" % rnd
    pipe.close()
    for b in room + [crops]:
        b.free()
