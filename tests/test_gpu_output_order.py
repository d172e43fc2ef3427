"""Pictures in display order through the pipeline's sink on the device (p264pipe_set_output_order): three streams of 5 x 4
macroblocks - B pictures with a VUI that gives depth 1, two B streams without VUI one behind the other (the second IDR picture
flushes eight pictures at once, and until then they stay in the frame store for up to 8 rounds while 16 other reconstructs run),
and a Baseline stream - into two sink buffers of exactly three pictures, so that the larger rounds and the final flush go out in
several deliveries.

The expected BYTES come from the road that exists without the option: the same three streams with output order off and the
decode-order sink, which records every (stream, decode index) picture (those pictures are pinned to the checkers elsewhere).  The
expected ORDER comes from tests/output_order_model.py.  Once with the plain I420 sink, once with the resized one (planar RGB,
float16, 32 x 24, antialiased)."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline
from tests import output_order_model as M
from tests import synth_cases
from tests.device_mem import DeviceBuffer
from tests.test_output_order_cpu import MB, REFS, b_stream

pytestmark = pytest.mark.gpu

FRAMES = (14, 16, 9)
CAPACITY = 3
SIZE, FMT, DTYPE = (32, 24), "rgbp", "f16"
SCALE = 1 / 255


@pytest.fixture(scope="module")
def streams():
    base = "--mbw %d --mbh %d --frames 9 --gop 4 --seed 21 --coded 10 --maxlevel 6" % MB
    return [b_stream(2, "1"), b_stream(2, None, frames=8, seed=11) + b_stream(2, None, frames=8, seed=12), open(synth_cases.generate(base), "rb").read()]


def model():
    """[[(stream, decode index)]] per delivery"""
    runs = [M.run(M.bframes_pictures(14, 2), 1, 2, REFS), M.run(M.bframes_pictures(8, 2) * 2, 16, 16, REFS), M.run(M.baseline_pictures(9, 4), 0, 16, 1)]
    rounds = [[run[0][r] if r < len(run[0]) else None for run in runs] for r in range(max(FRAMES))]
    return M.deliveries(rounds, [run[1] for run in runs], CAPACITY)


def run_pipeline(lib, streams, set_sink, per, ordered):
    """one run with the sink set_sink(pipe, callback, buffers) installs; returns ([(number, [(stream, decode index)], buffer, bytes)],
    the pipeline - still open - and its buffers)"""
    n = len(streams)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    if ordered:
        pipe.set_output_order()
    room = [DeviceBuffer(lib, CAPACITY * per) for _ in range(2)]
    seen = []

    def sink(number, which, dev, size):
        host = np.empty(len(which) * size, np.uint8)
        assert size == per and lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        who = [(g[0], g[2]) for g in pipe.delivery()] if ordered else [(s, number) for s in which]      # (decode order: round r brings picture r)
        assert [w[0] for w in who] == list(which)
        seen.append((number, who, dev, host))
    assert set_sink(pipe, sink, [(b.ptr, b.nbytes) for b in room]) == per
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and st["rounds"] == max(FRAMES)
    return seen, pipe, room


def check_deliveries(lib, streams, set_sink, per):
    plain, pipe, room = run_pipeline(lib, streams, set_sink, per, False)
    pipe.close()
    recorded = {w: host[k * per:(k + 1) * per] for _, who, _, host in plain for k, w in enumerate(who)}
    assert sorted(recorded) == [(s, i) for s in range(3) for i in range(FRAMES[s])]
    for b in room:
        b.free()
    seen, pipe, room = run_pipeline(lib, streams, set_sink, per, True)
    want = model()
    assert [d for d, _, _, _ in seen] == list(range(len(want)))
    assert [who for _, who, _, _ in seen] == want
    assert all(dev == room[d % 2].ptr for d, _, dev, _ in seen)                 # two buffers taking turns, by delivery
    assert any(len(w) == CAPACITY for w in want) and len(want) > max(FRAMES)     # (rounds and the flush were cut into pieces)
    for d, who, _, host in seen:
        for k, w in enumerate(who):
            assert np.array_equal(host[k * per:(k + 1) * per], recorded[w]), "delivery %d picture %d: stream %d decode index %d" % (d, k, w[0], w[1])
    return pipe, room, recorded


def test_display_order_through_the_plain_sink(lib, streams):
    w, h = MB[0] * 16, MB[1] * 16
    per = w * h * 3 // 2
    pipe, room, recorded = check_deliveries(lib, streams, lambda p, cb, bufs: p.set_sink("i420", cb, buffers=bufs), per)
    # the last DECODED picture of every stream is still what export_last and read_frame hand out
    last = DeviceBuffer(lib, 3 * per)
    pipe.export_last("i420", out=(last.ptr, 3 * per))
    got = last.host()
    for s in range(3):
        assert np.array_equal(got[s * per:(s + 1) * per], recorded[(s, FRAMES[s] - 1)]), "export_last, stream %d" % s
        y, u, v = pipe.read_frame(s)
        assert np.array_equal(np.concatenate([y.ravel(), u.ravel(), v.ravel()]), recorded[(s, FRAMES[s] - 1)]), "read_frame, stream %d" % s
    pipe.close()
    for b in room + [last]:
        b.free()


def test_display_order_through_the_resized_sink(lib, streams):
    per = 3 * SIZE[0] * SIZE[1] * 2
    pipe, room, _ = check_deliveries(lib, streams, lambda p, cb, bufs: p.set_sink_resized(SIZE, cb, FMT, DTYPE, scale=SCALE, buffers=bufs, filter="bilinear_aa"), per)
    pipe.close()
    for b in room:
        b.free()
