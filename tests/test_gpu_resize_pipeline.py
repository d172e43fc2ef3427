"""The pipeline's resized exits in device memory: a sink that receives every round's pictures resized (p264pipe_set_sink_resized) and
the last picture of every stream in one launch (p264pipe_export_last_resized).  The streams of tests/test_gpu_export_pipeline.py:
three cropped streams of 8 x 6 macroblocks, different content and length; every picture of every round must be what the stream
gives when it is decoded alone, its display window resized and converted by tests/resize_checker.py.  A pipeline has one sink:
setting the plain one afterwards replaces the resized one, and the other way round."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline
from tests import export_checker as X
from tests import resize_checker as R
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export_pipeline import FRAMES, WINDOW, decode_alone, make_streams

pytestmark = pytest.mark.gpu

SIZE = (50, 38)
NORM = ([1 / (255 * s) for s in (0.229, 0.224, 0.225)], [-m / s for m, s in zip((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))])


@pytest.fixture(scope="module")
def streams():
    return make_streams((8, 6), FRAMES, "0 3 0 2", 70)


@pytest.fixture(scope="module")
def alone(lib, streams):
    return decode_alone(lib, streams, (8, 6), FRAMES, WINDOW)


def collector(lib, rounds):
    def sink(rnd, which, dev, per):
        host = np.empty(len(which) * per, np.uint8)
        assert lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        rounds.append((rnd, list(which), dev, host))
    return sink


@pytest.mark.parametrize("fmt,dtype", [("nv12", "u8"), ("rgbp", "f32"), ("rgb24", "f16")])
def test_resized_sink_and_export_last(lib, streams, alone, fmt, dtype):
    n = len(streams)
    scale, bias = NORM if dtype != "u8" else (None, None)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    rounds = []
    per = R.frame_bytes(fmt, SIZE[0], SIZE[1], dtype)
    room = [DeviceBuffer(lib, n * per) for _ in range(2)]
    assert pipe.set_sink_resized(SIZE, collector(lib, rounds), fmt, dtype, scale=scale, bias=bias, buffers=[(b.ptr, b.nbytes) for b in room]) == per
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and st["rounds"] == max(FRAMES)
    assert [r[0] for r in rounds] == list(range(max(FRAMES)))
    assert [r[1] for r in rounds] == [[s for s in range(n) if FRAMES[s] > rnd] for rnd in range(max(FRAMES))]
    assert len({r[2] for r in rounds}) == 2 and all(rounds[r][2] == rounds[r % 2][2] for r in range(max(FRAMES)))      # two buffers taking turns
    for rnd, which, _, host in rounds:
        want = R.expected([alone[s][rnd] for s in which], fmt, WINDOW, SIZE, dtype, scale, bias)
        assert np.array_equal(host, want), "round %d" % rnd
    last = DeviceBuffer(lib, n * per + 16)
    pipe.export_last_resized(SIZE, fmt, dtype, scale=scale, bias=bias, out=(last.ptr, n * per))
    assert np.array_equal(last.host(), R.expected([f[-1] for f in alone], fmt, WINDOW, SIZE, dtype, scale, bias, total=n * per + 16))
    # the plain export of the same pictures is untouched by all this
    plain = DeviceBuffer(lib, n * X.frame_bytes("i420", WINDOW[2], WINDOW[3]))
    pipe.export_last("i420", out=(plain.ptr, plain.nbytes))
    assert np.array_equal(plain.host(), X.expected([f[-1] for f in alone], "i420", WINDOW))
    pipe.close()
    for b in room + [last, plain]:
        b.free()


def test_one_sink_either_kind_replaces_the_other(lib, streams, alone):
    n = len(streams)
    per_r, per_p = R.frame_bytes("rgbp", SIZE[0], SIZE[1]), X.frame_bytes("i420", WINDOW[2], WINDOW[3])
    room = [DeviceBuffer(lib, n * max(per_r, per_p)) for _ in range(2)]
    bufs = [(b.ptr, b.nbytes) for b in room]
    # resized, then plain: the run delivers plain pictures only
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    resized, plain = [], []
    pipe.set_sink_resized(SIZE, collector(lib, resized), buffers=bufs)
    assert pipe.set_sink("i420", collector(lib, plain), buffers=bufs) == per_p
    pipe.run()
    assert not resized and len(plain) == max(FRAMES)
    assert np.array_equal(plain[0][3], X.expected([alone[s][0] for s in plain[0][1]], "i420", WINDOW))
    pipe.close()
    # plain, then resized
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    resized, plain = [], []
    pipe.set_sink("i420", collector(lib, plain), buffers=bufs)
    assert pipe.set_sink_resized(SIZE, collector(lib, resized), buffers=bufs) == per_r
    pipe.run()
    assert not plain and len(resized) == max(FRAMES)
    assert np.array_equal(resized[-1][3], R.expected([alone[s][max(FRAMES) - 1] for s in resized[-1][1]], "rgbp", WINDOW, SIZE))
    pipe.close()
    for b in room:
        b.free()


def test_a_resized_sink_buffer_too_small_is_refused(lib, streams):
    pipe = Pipeline(streams, threads=2, device=0, lib=lib)
    per = R.frame_bytes("rgbp", SIZE[0], SIZE[1], "f16")
    room = [DeviceBuffer(lib, 3 * per) for _ in range(2)]
    with pytest.raises(RuntimeError):
        pipe.set_sink_resized(SIZE, lambda *a: None, "rgbp", "f16", scale=1 / 255, buffers=[(room[0].ptr, 3 * per), (room[1].ptr, 3 * per - 1)])
    with pytest.raises(RuntimeError):
        pipe.set_sink_resized((51, 38), lambda *a: None, buffers=[(room[0].ptr, 3 * per)])
    # a window that leaves the streams' frame is known at the first round: the run fails, nothing is written
    pipe.set_sink_resized(SIZE, lambda *a: None, "rgbp", "f16", scale=1 / 255, crop=(100, 0, 30, 92), buffers=[(room[0].ptr, 3 * per)])
    with pytest.raises(RuntimeError):
        pipe.run()
    assert np.all(room[0].host() == 0xA5)
    pipe.close()
    for b in room:
        b.free()
