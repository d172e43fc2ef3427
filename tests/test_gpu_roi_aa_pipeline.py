"""The pipeline's exit for per-picture windows with the antialiased filter (p264pipe_export_last_rois chooses p264hip_export_rois_aa by
the description's filter): after a run, and from inside the callback of a decode-order sink.  The streams of
tests/test_gpu_roi_pipeline.py; every crop must be tests/roi_aa_checker.py's on the pictures each stream gives when it is decoded
alone."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline
from tests import export_checker as X
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export_pipeline import FRAMES, WINDOW
from tests.test_gpu_roi_pipeline import NORM, SIZE, WIDE, alone, rows_of, streams  # noqa: F401  (alone, streams: the fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt,dtype", [("nv12", "u8"), ("rgbp", "f32")])
def test_export_last_rois_antialiased_after_a_run(lib, streams, alone, fmt, dtype):
    n = len(streams)
    scale, bias = NORM if dtype != "u8" else (None, None)
    pipe = Pipeline(streams, threads=n, device=0, lib=lib)
    per = R.frame_bytes(fmt, SIZE[0], SIZE[1], dtype)
    rows, model = rows_of([2, 0, 1, 2])
    out = DeviceBuffer(lib, len(rows) * per + 16)
    pipe.run()
    last = {(s, 0): alone[s][-1] for s in range(n)}
    pipe.export_last_rois(rows, SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(out.ptr, len(rows) * per), filter="bilinear_aa")
    want = KA.expected(model, last, SIZE, fmt, dtype, (235, 16, 240), scale, bias, total=len(rows) * per + 16)
    assert np.array_equal(out.host(), want)
    # the default is the plain filter, as before - and the two differ on these reductions
    out.fill(0xA5)
    pipe.export_last_rois(rows, SIZE, fmt, dtype, (235, 16, 240), scale, bias, out=(out.ptr, len(rows) * per))
    plain = K.expected(model, last, SIZE, fmt, dtype, (235, 16, 240), scale, bias, total=len(rows) * per + 16)
    assert np.array_equal(out.host(), plain) and not np.array_equal(plain, want)
    # a window more than 32 times its rectangle: refused, nothing written
    out.fill(0xA5)
    with pytest.raises(RuntimeError):
        pipe.export_last_rois([(0,) + WIDE, (1, 0, 0, 128, 96, 0, 0, 2, 2)], SIZE, fmt, dtype, scale=scale, bias=bias, out=(out.ptr, len(rows) * per), filter="bilinear_aa")
    assert np.all(out.host() == 0xA5)
    pipe.close()
    out.free()


def test_antialiased_crops_from_inside_a_decode_order_sink(lib, streams, alone):
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
        pipe.export_last_rois(rows, SIZE, "rgbp", "f16", scale=NORM[0], bias=NORM[1], out=(crops.ptr, len(rows) * per), filter="bilinear_aa")
        host = np.empty(len(which) * nbytes, np.uint8)
        assert lib.p264hip_copy_from_device(host.ctypes.data, dev, host.size) == 0
        rounds.append((rnd, list(which), host, crops.host(), model))
    assert pipe.set_sink("i420", sink, buffers=[(b.ptr, b.nbytes) for b in room]) == per_sink
    st = pipe.run()
    assert st["pictures"] == sum(FRAMES) and [r[0] for r in rounds] == list(range(max(FRAMES)))
    for rnd, which, host, got, model in rounds:
        assert np.array_equal(host, X.expected([alone[s][rnd] for s in which], "i420", WINDOW)), "the sink's buffer of round %d" % rnd
        now = {(s, 0): alone[s][rnd] for s in which}
        want = KA.expected(model, now, SIZE, "rgbp", "f16", K.FILL, NORM[0], NORM[1], total=2 * n * per + 16)
        assert np.array_equal(got, want), "the crops of round %d" % rnd
    pipe.close()
    for b in room + [crops]:
        b.free()
