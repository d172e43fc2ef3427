"""p264hip_export_frames on the MI355X: batches of frames out of the frame stores into device memory, cropped, as I420 / NV12 /
RGB24 / planar RGB.  The frames are random planes put there with write_frame (no decode needed); every test prefills the whole
destination with 0xA5 and compares ALL of it with tests/export_checker.py applied to the read_frame planes, so a byte written
outside the layout - between a row's end and the pitch, between pictures, in front of or behind the destination - fails it.

Frame 5 x 3 macroblocks: five strips (no multiple of the eight a wavefront takes), 48 rows (two tile rows of 32); windows that are the
frame, that start or end inside a strip, that start below the first row group, and one of 2 x 2 samples."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from p264decoder_amd.recon import P264Error
from tests import export_checker as X
from tests import synth_cases
from tests.device_mem import DeviceBuffer
from tests.hip_harness import reconstructor

pytestmark = pytest.mark.gpu

MB_W, MB_H, STREAMS, SLOTS = 5, 3, 3, 2
WINDOWS = [(0, 0, 80, 48), (0, 0, 80, 40), (2, 2, 62, 30), (16, 10, 48, 22), (18, 0, 62, 48), (6, 46, 2, 2)]
KINDS = [("i420", "bt601", False), ("nv12", "bt601", False)] + [(f, m, r) for f in ("rgb24", "rgbp") for m in ("bt601", "bt709") for r in (False, True)]
# (streams, slots) of a call: one picture; five with a repeated entry and out of order; all six frames
BATCHES = [([2], [1]), ([2, 0, 1, 2, 0], [1, 0, 1, 1, 1]), ([0, 0, 1, 1, 2, 2], [0, 1, 0, 1, 0, 1])]
TAIL = 48          # bytes of the destination behind the last picture: they stay 0xA5


@pytest.fixture(scope="module")
def store(lib):
    """a context whose six frames hold random planes, and those planes as read_frame returns them"""
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        g = np.random.default_rng(2640)
        w, h = MB_W * 16, MB_H * 16
        for s in range(STREAMS):
            for k in range(SLOTS):
                # (full range of every plane: the RGB clips are reached)
                hip.write_frame(s, k, g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8))
        planes = {(s, k): hip.read_frame(s, k) for s in range(STREAMS) for k in range(SLOTS)}
        yield hip, planes


def run(hip, planes, streams, slots, fmt, crop, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """one export into a prefilled destination; returns (what the device holds, what the checker says it holds)"""
    per = X.frame_bytes(fmt, crop[2], crop[3], pitch)
    total = offset + (len(streams) - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_frames(streams, slots, fmt, crop, matrix, full, pitch, out=(dst.ptr + offset, total - offset - TAIL), frame_stride=stride)
    want = X.expected([planes[(s, k)] for s, k in zip(streams, slots)], fmt, crop, matrix, full, pitch, stride, offset, total)
    got = dst.host()
    dst.free()
    return got, want


@pytest.mark.parametrize("fmt,matrix,full", KINDS)
def test_every_window_pitch_and_alignment(store, fmt, matrix, full):
    hip, planes = store
    n = 0
    for crop in WINDOWS:
        tight = X.tight_pitch(fmt, crop[2])
        for pitch in (0, tight + 16, tight + 2):
            for offset in (0, 1, 4):
                streams, slots = BATCHES[n % 3]
                per = X.frame_bytes(fmt, crop[2], crop[3], pitch)
                stride = 0 if (n // 3) % 2 == 0 else per + 7          # (3 batches x 2 strides: every pair comes round in six cases)
                n += 1
                got, want = run(hip, planes, streams, slots, fmt, crop, matrix, full, pitch, stride, offset)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, "%s window %s pitch %d offset %d stride %d, %d pictures: %d bytes differ, the first at %d (%d, want %d)" % (
                    fmt, crop, pitch, offset, stride, len(streams), bad.size, bad[0], got[bad[0]], want[bad[0]])


def test_i420_of_the_full_frame_is_the_planar_road(store):
    hip, planes = store
    crop = (0, 0, MB_W * 16, MB_H * 16)
    for (s, k) in planes:
        got, want = run(hip, planes, [s], [k], "i420", crop)
        assert np.array_equal(got, want)
        dev, nbytes = hip.frame_planar_device(s, k)
        hip.sync()
        road = np.empty(nbytes, np.uint8)
        assert hip.lib.p264hip_copy_from_device(road.ctypes.data, dev, nbytes) == 0
        assert nbytes == got.size - TAIL and np.array_equal(got[:nbytes], road)


def test_more_pictures_than_a_grid_dimension(lib):
    """70 000 pictures of a 1 x 1 macroblock context (27 MB of I420): the launch is chunked at 65 535"""
    with reconstructor(lib, 1, 1, n_streams=2, slots=2, max_pictures=1) as hip:
        g = np.random.default_rng(7)
        for s in range(2):
            for k in range(2):
                hip.write_frame(s, k, g.integers(0, 256, (16, 16), np.uint8), g.integers(0, 256, (8, 8), np.uint8), g.integers(0, 256, (8, 8), np.uint8))
        planes = {(s, k): hip.read_frame(s, k) for s in range(2) for k in range(2)}
        n = 70000
        which = (np.arange(n) * 7 + np.arange(n) // 65535) % 4              # (stream, slot) = (which >> 1, which & 1); the pattern shifts at the seam
        dst = DeviceBuffer(lib, n * 384 + TAIL)
        hip.export_frames((which >> 1).tolist(), (which & 1).tolist(), "i420", out=(dst.ptr, n * 384))
        got = dst.host()
        dst.free()
        four = np.stack([X.expected([planes[(w >> 1, w & 1)]], "i420", (0, 0, 16, 16)) for w in range(4)])
        assert np.array_equal(got[:n * 384].reshape(n, 384), four[which])
        assert np.all(got[n * 384:] == 0xA5)


def test_an_export_runs_behind_the_reconstruct_before_it(lib):
    data = open(synth_cases.generate("--mbw 5 --mbh 3 --frames 3 --gop 0 --seed 31 --coded 30 --maxlevel 8"), "rb").read()
    parser = Parser(lib=lib)
    pics = parser.parse_stream(data)
    assert len(pics) == 3
    with reconstructor(lib, MB_W, MB_H, n_streams=1, slots=parser.slots, max_pictures=1) as hip:
        dst = DeviceBuffer(lib, 80 * 48 * 3 // 2)
        for p in pics:
            hip.submit(0, p)                                                   # asynchronous: nothing waits for the kernels ...
            hip.export_frames([0], [p.desc.dst_slot], "i420", out=(dst.ptr, dst.nbytes), sync=True)   # ... but the export is queued behind them
            want = X.expected([hip.read_frame(0, p.desc.dst_slot)], "i420", (0, 0, 80, 48))
            assert np.array_equal(dst.host(), want)
        dst.free()
        assert len({bytes(hip.read_frame(0, p.desc.dst_slot)[0]) for p in pics[:2]}) == 2      # (the pictures differ: a stale frame would show)


def test_refusals_queue_nothing(store):
    hip, planes = store
    lib = hip.lib
    crop = (2, 2, 62, 30)
    per = X.frame_bytes("i420", 62, 30)
    total = 2 * per + TAIL
    dst = DeviceBuffer(lib, total)
    ptr = dst.ptr
    two = (C.c_int * 2)(0, 1)

    def call(e, streams=two, slots=two, n=2, d=ptr, cap=2 * per, ctx=hip.h):
        return lib.p264hip_export_frames(ctx, streams, slots, n, C.byref(e) if e is not None else None, d, cap)

    def E(fmt="i420", crop=crop, **kw):
        return N.export_desc(fmt, crop, None, **kw)
    assert call(E()) == 0
    hip.sync()
    dst.fill(0xA5)
    refused = [
        # a null argument, n < 1, a stream or slot out of range
        lambda: call(E(), ctx=None), lambda: call(E(), streams=None), lambda: call(E(), slots=None), lambda: call(None), lambda: call(E(), d=None),
        lambda: call(E(), n=0), lambda: call(E(), n=-1),
        lambda: call(E(), streams=(C.c_int * 2)(0, STREAMS)), lambda: call(E(), streams=(C.c_int * 2)(-1, 0)),
        lambda: call(E(), slots=(C.c_int * 2)(0, SLOTS)), lambda: call(E(), slots=(C.c_int * 2)(0, -1)),
        # an unknown format or matrix, matrix / full_range on a YUV format
        lambda: call(E(fmt=4), cap=1 << 20), lambda: call(E("rgbp", matrix=2), cap=1 << 20), lambda: call(E("i420", matrix="bt709")), lambda: call(E("nv12", full_range=True)),
        # a window with an odd member, or one that leaves the frame
        lambda: call(E(crop=(1, 2, 62, 30))), lambda: call(E(crop=(2, 3, 62, 30))), lambda: call(E(crop=(2, 2, 61, 30))), lambda: call(E(crop=(2, 2, 62, 29))),
        lambda: call(E(crop=(20, 2, 62, 30))), lambda: call(E(crop=(2, 20, 62, 30))), lambda: call(E(crop=(2, 2, 0, 30))),
        # a pitch below the tight one, an odd one for I420; a frame_stride below the picture's bytes; a destination too small
        lambda: call(E(pitch=60)), lambda: call(E(pitch=63)), lambda: call(E("rgb24", pitch=184), cap=1 << 20),
        lambda: call(E(frame_stride=per - 1)), lambda: call(E(), cap=2 * per - 1), lambda: call(E(frame_stride=per + 8), cap=2 * per + 7),
    ]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_frames:"), i
    hip.sync()
    assert np.all(dst.host() == 0xA5)
    # ... and the wrapper raises for them
    with pytest.raises(P264Error):
        hip.export_frames([0, STREAMS], [0, 0], out=(ptr, total))
    with pytest.raises(P264Error):
        hip.export_frames([0], [0], "i420", (2, 2, 62, 30), pitch=63, out=(ptr, total))
    assert np.all(dst.host() == 0xA5)
    assert call(E()) == 0
    hip.sync()
    assert np.array_equal(dst.host(), X.expected([planes[(0, 0)], planes[(1, 1)]], "i420", crop, total=total))
    dst.free()


TORCH_CHILD = r"""
import sys
import torch                                   # first: the library then shares torch's HIP runtime
if not torch.cuda.is_available():
    print("no device")
    sys.exit(0)
sys.path.insert(0, %r)
import numpy as np
from p264decoder_amd import HipReconstructor
from tests import export_checker as X
hip = HipReconstructor(5, 3, n_streams=3, slots=2, max_pictures=1)
g = np.random.default_rng(99)
for s in range(3):
    for k in range(2):
        hip.write_frame(s, k, g.integers(0, 256, (48, 80), np.uint8), g.integers(0, 256, (24, 40), np.uint8), g.integers(0, 256, (24, 40), np.uint8))
planes = {(s, k): hip.read_frame(s, k) for s in range(3) for k in range(2)}
streams, slots = [1, 2, 0], [1, 0, 1]
frames = [planes[(s, k)] for s, k in zip(streams, slots)]
for fmt, shape in (("i420", (3, 72, 80)), ("nv12", (3, 72, 80)), ("rgb24", (3, 48, 80, 3)), ("rgbp", (3, 3, 48, 80))):
    matrix = "bt709" if fmt.startswith("rgb") else "bt601"
    out = hip.export_frames(streams, slots, fmt, matrix=matrix)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == shape, (fmt, out.shape)
    assert np.array_equal(out.cpu().numpy().reshape(-1), X.expected(frames, fmt, (0, 0, 80, 48), matrix)), fmt
    # the documented shapes mean what they say: plane / channel c of picture i
    if fmt == "rgbp":
        (r, gr, b), _ = X.rgb(frames[1][0], np.repeat(np.repeat(frames[1][1], 2, 0), 2, 1), np.repeat(np.repeat(frames[1][2], 2, 0), 2, 1), "bt709")
        assert np.array_equal(out[1, 1].cpu().numpy(), gr)
    if fmt == "rgb24":
        (r, gr, b), _ = X.rgb(frames[0][0], np.repeat(np.repeat(frames[0][1], 2, 0), 2, 1), np.repeat(np.repeat(frames[0][2], 2, 0), 2, 1), "bt709")
        assert np.array_equal(out[0, :, :, 2].cpu().numpy(), b)
    if fmt == "i420":
        assert np.array_equal(out[2, :48].cpu().numpy(), frames[2][0])
    # an existing tensor is filled in place, here with a window
    mine = torch.full((3, X.frame_bytes(fmt, 48, 22)), 0xA5, dtype=torch.uint8, device="cuda")
    back = hip.export_frames(streams, slots, fmt, (16, 10, 48, 22), out=mine)
    assert back is mine
    assert np.array_equal(mine.cpu().numpy().reshape(-1), X.expected(frames, fmt, (16, 10, 48, 22))), fmt
hip.close()
print("ok")
"""


def test_torch_tensors():
    """out=None returns a tensor of the documented shape on the device, out= an existing tensor is filled in place.  In a process of
    its own, which imports torch BEFORE the library is loaded (one HIP runtime per process)."""
    import os
    import subprocess
    import sys
    import importlib.util
    if importlib.util.find_spec("torch") is None:          # (looked for, NOT imported: this process keeps the one HIP runtime it has)
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD % root], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if r.returncode == 0 and r.stdout.strip().endswith("no device"):
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]
