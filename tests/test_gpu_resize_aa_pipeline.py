"""The pipeline's resized exits with the antialiased filter: the streams of tests/test_gpu_export_pipeline.py (three cropped streams
of 8 x 6 macroblocks) through Pipeline.set_sink_resized(filter="bilinear_aa") and export_last_resized(filter="bilinear_aa") at 34 x 18
planar float16.  Every round's buffer must be tests/resize_aa_checker.py applied to the planes the stream gives when it is decoded
alone.  A pipeline has one sink: a filter-0 sink set afterwards replaces the antialiased one and delivers filter-0 bytes."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline
from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export_pipeline import FRAMES, WINDOW, decode_alone, make_streams
from tests.test_gpu_resize_pipeline import NORM, collector

pytestmark = pytest.mark.gpu

SIZE, FMT, DTYPE = (34, 18), "rgbp", "f16"


@pytest.fixture(scope="module")
def streams():
    return make_streams((8, 6), FRAMES, "0 3 0 2", 70)


@pytest.fixture(scope="module")
def alone(lib, streams):
    return decode_alone(lib, streams, (8, 6), FRAMES, WINDOW)


def test_antialiased_sink_and_export_last_then_a_bilinear_sink(lib, streams, alone):
    n = len(streams)
    scale, bias = NORM
    per = R.frame_bytes(FMT, SIZE[0], SIZE[1], DTYPE)
    room = [DeviceBuffer(lib, n * per) for _ in range(2)]
    bufs = [(b.ptr, b.nbytes) for b in room]
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    rounds = []
    assert pipe.set_sink_resized(SIZE, collector(lib, rounds), FMT, DTYPE, scale=scale, bias=bias, buffers=bufs, filter="bilinear_aa") == per
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and [r[0] for r in rounds] == list(range(max(FRAMES)))
    differs = False
    for rnd, which, _, host in rounds:
        frames = [alone[s][rnd] for s in which]
        assert np.array_equal(host, A.expected_aa(frames, FMT, WINDOW, SIZE, DTYPE, scale, bias)), "round %d" % rnd
        differs |= not np.array_equal(host, R.expected(frames, FMT, WINDOW, SIZE, DTYPE, scale, bias))
    assert differs                                           # (3.6 : 1 and 5.1 : 1: the two filters do not give the same bytes)
    last = DeviceBuffer(lib, n * per + 16)
    pipe.export_last_resized(SIZE, FMT, DTYPE, scale=scale, bias=bias, out=(last.ptr, n * per), filter="bilinear_aa")
    assert np.array_equal(last.host(), A.expected_aa([f[-1] for f in alone], FMT, WINDOW, SIZE, DTYPE, scale, bias, total=n * per + 16))
    # the same pipeline with filter 0: the last pictures, as names and as numbers
    for flt in ("bilinear", 0):
        last.fill(0xA5)
        pipe.export_last_resized(SIZE, FMT, DTYPE, scale=scale, bias=bias, out=(last.ptr, n * per), filter=flt)
        assert np.array_equal(last.host(), R.expected([f[-1] for f in alone], FMT, WINDOW, SIZE, DTYPE, scale, bias, total=n * per + 16))
    pipe.close()
    # an antialiased sink, then a filter-0 sink on the same pipeline: the run delivers filter-0 pictures only
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    first, second = [], []
    pipe.set_sink_resized(SIZE, collector(lib, first), FMT, DTYPE, scale=scale, bias=bias, buffers=bufs, filter="bilinear_aa")
    assert pipe.set_sink_resized(SIZE, collector(lib, second), FMT, DTYPE, scale=scale, bias=bias, buffers=bufs) == per
    pipe.run()
    assert not first and len(second) == max(FRAMES)
    for rnd, which, _, host in second:
        assert np.array_equal(host, R.expected([alone[s][rnd] for s in which], FMT, WINDOW, SIZE, DTYPE, scale, bias)), "round %d" % rnd
    pipe.close()
    for b in room + [last]:
        b.free()


def test_a_reduction_above_the_limit_is_refused_by_the_sink(lib, streams):
    pipe = Pipeline(streams, threads=2, device=0, lib=lib)
    room = DeviceBuffer(lib, 1 << 16)
    with pytest.raises(RuntimeError):
        pipe.set_sink_resized((2, 2), lambda *a: None, buffers=[(room.ptr, room.nbytes)], filter="bilinear_aa")        # 122 : 2
    with pytest.raises(KeyError):
        pipe.set_sink_resized(SIZE, lambda *a: None, buffers=[(room.ptr, room.nbytes)], filter="box")
    pipe.close()
    room.free()
