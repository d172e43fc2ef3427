"""The pipeline's exits in device memory: a sink that receives every round's pictures (p264pipe_set_sink), the last picture of every
stream in one launch (p264pipe_export_last) and the display window (p264pipe_crop).  Three cropped streams of different content and
length; every picture of every round must be what the stream gives when it is decoded alone, cropped and converted by
tests/export_checker.py.  Once more with two streams of 19 x 4 macroblocks, whose window has three luma tile columns and
two I420 chroma tile columns (kernel_export.h; tests/test_gpu_export_wide.py has the windows one by one)."""
import numpy as np
import pytest

from p264decoder_amd import Parser, Pipeline
from tests import export_checker as X
from tests import synth_cases
from tests.device_mem import DeviceBuffer
from tests.hip_harness import reconstructor

pytestmark = pytest.mark.gpu

FRAMES = (6, 6, 4)
WINDOW = (0, 0, 8 * 16 - 6, 6 * 16 - 4)                    # --crop 0 3 0 2
WIDE_FRAMES = (3, 2)
WIDE_MB = (19, 4)
WIDE_WINDOW = (2, 0, 19 * 16 - 8, 4 * 16 - 4)              # --crop 1 3 0 2: strips 0 .. 18


def make_streams(mb, frames, crop, seed):
    return [open(synth_cases.generate("--mbw %d --mbh %d --frames %d --gop 0 --seed %d --coded 25 --maxlevel 8 --crop %s" % (mb[0], mb[1], n, seed + i, crop)), "rb").read()
            for i, n in enumerate(frames)]


def decode_alone(lib, streams, mb, frames, window):
    """[stream][picture] -> (y, u, v): every stream decoded by itself"""
    out = []
    for data in streams:
        parser = Parser(lib=lib)
        pics = parser.parse_stream(data)
        assert parser.crop == window
        with reconstructor(lib, mb[0], mb[1], n_streams=1, slots=parser.slots, max_pictures=1) as hip:
            got = []
            for p in pics:
                hip.submit(0, p)
                got.append(hip.read_frame(0, p.desc.dst_slot))
        out.append(got)
    assert tuple(len(f) for f in out) == frames
    return out


@pytest.fixture(scope="module")
def streams():
    return make_streams((8, 6), FRAMES, "0 3 0 2", 70)


@pytest.fixture(scope="module")
def alone(lib, streams):
    return decode_alone(lib, streams, (8, 6), FRAMES, WINDOW)


def sink_and_export_last(lib, streams, alone, fmt, frames, window):
    n = len(streams)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    assert pipe.crop() is None                                # nothing parsed yet
    rounds = []

    def sink(rnd, which, dev, per):
        host = np.empty(len(which) * per, np.uint8)
        assert lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        rounds.append((rnd, list(which), dev, host))
    per = X.frame_bytes(fmt, window[2], window[3])
    room = [DeviceBuffer(lib, n * per) for _ in range(2)]
    assert pipe.set_sink(fmt, sink, buffers=[(b.ptr, b.nbytes) for b in room]) == per
    st = pipe.run()
    assert st["pictures"] == sum(frames) and st["rounds"] == max(frames)
    assert pipe.crop() == window
    assert [r[0] for r in rounds] == list(range(max(frames)))
    assert [r[1] for r in rounds] == [[s for s in range(n) if frames[s] > rnd] for rnd in range(max(frames))]
    assert len({r[2] for r in rounds}) == 2 and all(rounds[r][2] == rounds[r % 2][2] for r in range(max(frames)))      # two buffers taking turns
    for rnd, which, _, host in rounds:
        want = X.expected([alone[s][rnd] for s in which], fmt, window)
        assert np.array_equal(host, want), "round %d" % rnd
    last = DeviceBuffer(lib, n * per + 16)
    pipe.export_last(fmt, out=(last.ptr, n * per))
    assert np.array_equal(last.host(), X.expected([f[-1] for f in alone], fmt, window, total=n * per + 16))
    pipe.close()
    for b in room + [last]:
        b.free()


@pytest.mark.parametrize("fmt", ["i420", "rgb24"])
def test_sink_and_export_last(lib, streams, alone, fmt):
    assert [[s for s in range(3) if FRAMES[s] > rnd] for rnd in range(6)] == [[0, 1, 2]] * 4 + [[0, 1]] * 2
    sink_and_export_last(lib, streams, alone, fmt, FRAMES, WINDOW)


@pytest.fixture(scope="module")
def wide(lib):
    streams = make_streams(WIDE_MB, WIDE_FRAMES, "1 3 0 2", 75)
    return streams, decode_alone(lib, streams, WIDE_MB, WIDE_FRAMES, WIDE_WINDOW)


@pytest.mark.parametrize("fmt", ["i420", "nv12", "rgb24"])
def test_sink_and_export_last_of_a_wide_stream(lib, wide, fmt):
    """19 x 4 macroblocks with --crop 1 3 0 2: the window touches all 19 strips - luma tile columns of 8 + 8 + 3, ten I420 strip pairs
    whose last has one strip - and begins inside a strip, so the pipeline's road passes a multi-column export"""
    from tests.test_gpu_export_wide import reach
    assert reach(WIDE_WINDOW)[:3] == (0, 19, 3) and reach(WIDE_WINDOW)[4:6] == (10, 2)
    sink_and_export_last(lib, wide[0], wide[1], fmt, WIDE_FRAMES, WIDE_WINDOW)


def test_a_sink_buffer_too_small_is_refused(lib, streams):
    pipe = Pipeline(streams, threads=2, device=0, lib=lib)
    per = X.frame_bytes("i420", WINDOW[2], WINDOW[3])
    room = [DeviceBuffer(lib, 3 * per) for _ in range(2)]
    with pytest.raises(RuntimeError):
        pipe.set_sink("i420", lambda *a: None, buffers=[(room[0].ptr, 3 * per), (room[1].ptr, 3 * per - 1)])
    # a window that leaves the streams' frame is known at the first round: the run fails, nothing is written
    pipe.set_sink("i420", lambda *a: None, crop=(100, 0, 30, 92), buffers=[(room[0].ptr, 3 * per)])
    with pytest.raises(RuntimeError):
        pipe.run()
    assert np.all(room[0].host() == 0xA5)
    pipe.close()
    for b in room:
        b.free()
