"""The pipeline's exits in device memory: a sink that receives every round's pictures (p264pipe_set_sink), the last picture of every
stream in one launch (p264pipe_export_last) and the display window (p264pipe_crop).  Three cropped streams of different content and
length; every picture of every round must be what the stream gives when it is decoded alone, cropped and converted by
tests/export_checker.py."""
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


@pytest.fixture(scope="module")
def streams():
    return [open(synth_cases.generate("--mbw 8 --mbh 6 --frames %d --gop 0 --seed %d --coded 25 --maxlevel 8 --crop 0 3 0 2" % (n, 70 + i)), "rb").read()
            for i, n in enumerate(FRAMES)]


@pytest.fixture(scope="module")
def alone(lib, streams):
    """[stream][picture] -> (y, u, v): every stream decoded by itself"""
    out = []
    for data in streams:
        parser = Parser(lib=lib)
        pics = parser.parse_stream(data)
        assert parser.crop == WINDOW
        with reconstructor(lib, 8, 6, n_streams=1, slots=parser.slots, max_pictures=1) as hip:
            frames = []
            for p in pics:
                hip.submit(0, p)
                frames.append(hip.read_frame(0, p.desc.dst_slot))
        out.append(frames)
    assert tuple(len(f) for f in out) == FRAMES
    return out


@pytest.mark.parametrize("fmt", ["i420", "rgb24"])
def test_sink_and_export_last(lib, streams, alone, fmt):
    pipe = Pipeline(streams, threads=3, device=0, lib=lib)
    assert pipe.crop() is None                                # nothing parsed yet
    rounds = []

    def sink(rnd, which, dev, per):
        host = np.empty(len(which) * per, np.uint8)
        assert lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        rounds.append((rnd, list(which), dev, host))
    per = X.frame_bytes(fmt, WINDOW[2], WINDOW[3])
    room = [DeviceBuffer(lib, 3 * per) for _ in range(2)]
    assert pipe.set_sink(fmt, sink, buffers=[(b.ptr, b.nbytes) for b in room]) == per
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and st["rounds"] == max(FRAMES)
    assert pipe.crop() == WINDOW
    assert [r[0] for r in rounds] == list(range(6))
    assert [r[1] for r in rounds] == [[0, 1, 2]] * 4 + [[0, 1]] * 2
    assert len({r[2] for r in rounds}) == 2 and all(rounds[r][2] == rounds[r % 2][2] for r in range(6))      # two buffers taking turns
    for rnd, which, _, host in rounds:
        want = X.expected([alone[s][rnd] for s in which], fmt, WINDOW)
        assert np.array_equal(host, want), "round %d" % rnd
    last = DeviceBuffer(lib, 3 * per + 16)
    pipe.export_last(fmt, out=(last.ptr, 3 * per))
    assert np.array_equal(last.host(), X.expected([f[-1] for f in alone], fmt, WINDOW, total=3 * per + 16))
    pipe.close()
    for b in room + [last]:
        b.free()


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
