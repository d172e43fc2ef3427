"""p264hip_export_resized on the MI355X: batches of frames out of the frame stores into device memory, a window of each resized by
the fixed-point bilinear filter of include/p264hip.h, as I420 / NV12 / RGB24 / planar RGB bytes or - the RGB formats - as float16 /
float32 after a scale and a bias.  The fixture is tests/test_gpu_export.py's: 5 x 3 macroblocks, 3 streams x 2 slots of random
full-range planes put there with write_frame.  Every test prefills the whole destination with 0xA5 and compares ALL of it, floats
as bytes, with tests/resize_checker.py applied to the read_frame planes: a byte written outside the layout fails it.

Windows: the frame; two that start and end inside strips; one of 2 x 2 samples, where every tap clamps.  Output sizes: the window
itself (the filter must return the source), half of it where that is even (exactly the mean of four), 34 x 18 (reducing; 17 chroma
samples: the last lane of a row holds one), 162 x 98 (enlarging; 41 lanes of a row, the last with two samples), 2 x 2 and 6 x 70."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from p264decoder_amd.recon import P264Error
from tests import export_checker as X
from tests import resize_checker as R
from tests.device_mem import DeviceBuffer
from tests.hip_harness import reconstructor
from tests.test_gpu_export import BATCHES, KINDS, MB_H, MB_W, SLOTS, STREAMS, TAIL, WINDOWS as EXPORT_WINDOWS, run as run_export

pytestmark = pytest.mark.gpu

WINDOWS = [(0, 0, 80, 48), (2, 2, 62, 30), (16, 10, 48, 22), (6, 46, 2, 2)]
SIZES = [None, "half", (34, 18), (162, 98), (2, 2), (6, 70)]
# (format, dtype): the eight kernel instances
INSTANCES = [("i420", "u8"), ("nv12", "u8"), ("rgb24", "u8"), ("rgbp", "u8"), ("rgb24", "f16"), ("rgbp", "f16"), ("rgb24", "f32"), ("rgbp", "f32")]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALES = [((1 / 255,) * 3, (0.0,) * 3), (tuple(1 / (255 * s) for s in STD), tuple(-m / s for m, s in zip(MEAN, STD)))]
RGB_KINDS = [("bt601", False), ("bt709", True), ("bt709", False), ("bt601", True)]
ELEM = {"u8": 1, "f16": 2, "f32": 4}


def cases():
    """(window, output size) of every test below"""
    out = []
    for crop in WINDOWS:
        for size in SIZES:
            if size is None:
                size = crop[2:]
            elif size == "half":
                if crop[2] % 4 or crop[3] % 4:
                    continue
                size = (crop[2] // 2, crop[3] // 2)
            if (crop, size) not in out:
                out.append((crop, size))
    return out


@pytest.fixture(scope="module")
def store(lib):
    """a context whose six frames hold random planes, and those planes as read_frame returns them"""
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        g = np.random.default_rng(2650)
        w, h = MB_W * 16, MB_H * 16
        for s in range(STREAMS):
            for k in range(SLOTS):
                hip.write_frame(s, k, g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8))
        planes = {(s, k): hip.read_frame(s, k) for s in range(STREAMS) for k in range(SLOTS)}
        yield hip, planes


def run(hip, planes, streams, slots, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """one resized export into a prefilled destination; returns (what the device holds, what the checker says it holds)"""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    total = offset + (len(streams) - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_resized(streams, slots, size, fmt, dtype, crop, scale, bias, matrix, full, pitch, stride, out=(dst.ptr + offset, total - offset - TAIL))
    want = R.expected([planes[(s, k)] for s, k in zip(streams, slots)], fmt, crop, size, dtype, scale, bias, matrix, full, pitch, stride, offset, total)
    got = dst.host()
    dst.free()
    return got, want


def sweep(hip, planes, fmt, dtype, pairs, batches):
    """every (window, size) of `pairs` once, rotating pitch, destination offset, batch, frame stride, matrix / range and scale set"""
    elem = ELEM[dtype]
    n = 0
    for crop, size in pairs:
        tight = R.tight_pitch(fmt, size[0], dtype)
        pitch = (0, tight + 16, tight + 2 * elem)[n % 3]
        if fmt == "i420" and pitch % 2:
            pitch += 1
        offset = (0, elem, 4)[(n // 3) % 3]
        streams, slots = batches[(n + n // 9) % 3]
        per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
        stride = 0 if (n // 2) % 2 == 0 else per + 8
        matrix, full = RGB_KINDS[n % 4] if fmt.startswith("rgb") else ("bt601", False)
        scale, bias = SCALES[(n // 4) % 2] if dtype != "u8" else (None, None)
        n += 1
        got, want = run(hip, planes, streams, slots, fmt, crop, size, dtype, scale, bias, matrix, full, pitch, stride, offset)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s %s window %s to %s, %s %s, pitch %d offset %d stride %d, %d pictures: %d bytes differ, the first at %d (%d, want %d)" % (
            fmt, dtype, crop, size, matrix, full, pitch, offset, stride, len(streams), bad.size, bad[0], got[bad[0]], want[bad[0]])
    return n


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_every_window_size_pitch_and_alignment(store, fmt, dtype):
    hip, planes = store
    pairs = cases()
    assert len(pairs) == 20 and ((0, 0, 80, 48), (40, 24)) in pairs and ((6, 46, 2, 2), (2, 2)) in pairs
    # twice, the second time one step further round: 40 calls meet every pitch with every offset, both strides and every batch
    assert sweep(hip, planes, fmt, dtype, pairs + pairs[1:] + pairs[:1], BATCHES) == 40


def test_output_size_equal_to_the_window_is_the_plain_export(store):
    """the ten kinds of tests/test_gpu_export.py at its six windows: p264hip_export_resized with width x height = the window writes
    the bytes p264hip_export_frames writes"""
    hip, planes = store
    n = 0
    for fmt, matrix, full in KINDS:
        for crop in EXPORT_WINDOWS:
            tight = X.tight_pitch(fmt, crop[2])
            pitch = (0, tight + 16, tight + 2)[n % 3]
            offset = (0, 1, 4)[(n // 3) % 3]
            streams, slots = BATCHES[n % 3]
            n += 1
            plain, want = run_export(hip, planes, streams, slots, fmt, crop, matrix, full, pitch, 0, offset)
            got, _ = run(hip, planes, streams, slots, fmt, crop, crop[2:], "u8", None, None, matrix, full, pitch, 0, offset)
            assert np.array_equal(plain, want) and np.array_equal(got, plain), (fmt, matrix, full, crop, pitch, offset)


def test_refusals_queue_nothing(store):
    hip, planes = store
    lib = hip.lib
    crop, size = (2, 2, 62, 30), (34, 18)
    per = R.frame_bytes("rgbp", 34, 18, "f16")
    total = 2 * per + TAIL
    dst = DeviceBuffer(lib, total)
    ptr = dst.ptr
    two = (C.c_int * 2)(0, 1)

    def call(r, streams=two, slots=two, n=2, d=ptr, cap=2 * per, ctx=hip.h):
        return lib.p264hip_export_resized(ctx, streams, slots, n, C.byref(r) if r is not None else None, d, cap)

    def D(fmt="rgbp", size=size, crop=crop, dtype="f16", scale=1 / 255, **kw):
        return N.resize_desc(fmt, size, crop, None, dtype, scale, **kw)
    assert call(D()) == 0
    hip.sync()
    dst.fill(0xA5)
    refused = [
        lambda: call(D(), ctx=None), lambda: call(D(), streams=None), lambda: call(D(), slots=None), lambda: call(None), lambda: call(D(), d=None),
        lambda: call(D(), n=0), lambda: call(D(), streams=(C.c_int * 2)(0, STREAMS)), lambda: call(D(), slots=(C.c_int * 2)(0, -1)),
        lambda: call(D(fmt=4)), lambda: call(D(matrix=2)), lambda: call(D("i420")), lambda: call(D(dtype=3)), lambda: call(D(filter=1)),
        lambda: call(D(dtype="u8")), lambda: call(D(scale=float("nan"))), lambda: call(D(bias=float("inf"))),
        lambda: call(D(crop=(1, 2, 62, 30))), lambda: call(D(crop=(20, 2, 62, 30))), lambda: call(D(size=(33, 18))), lambda: call(D(size=(34, 0))),
        lambda: call(D(size=(16386, 2))), lambda: call(D(pitch=66)), lambda: call(D(pitch=71)),
        lambda: call(D(frame_stride=per - 2)), lambda: call(D(frame_stride=per + 1)), lambda: call(D(), cap=2 * per - 1),
        lambda: call(D(frame_stride=per + 8), cap=2 * per + 7), lambda: call(D(), d=ptr + 1, cap=2 * per),
    ]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_resized:"), i
    hip.sync()
    assert np.all(dst.host() == 0xA5)
    with pytest.raises(P264Error):
        hip.export_resized([0, STREAMS], [0, 0], size, out=(ptr, total))
    with pytest.raises(P264Error):
        hip.export_resized([0], [0], size, "nv12", "f32", out=(ptr, total))
    assert np.all(dst.host() == 0xA5)
    assert call(D()) == 0
    hip.sync()
    assert np.array_equal(dst.host(), R.expected([planes[(0, 0)], planes[(1, 1)]], "rgbp", crop, size, "f16", 1 / 255, None, total=total))
    dst.free()


def test_more_pictures_than_a_grid_dimension(lib):
    """70 000 pictures of a 1 x 1 macroblock context, 16 x 16 to 4 x 4 NV12 (24 bytes each): the launch is chunked at 65 535"""
    with reconstructor(lib, 1, 1, n_streams=2, slots=2, max_pictures=1) as hip:
        g = np.random.default_rng(8)
        for s in range(2):
            for k in range(2):
                hip.write_frame(s, k, g.integers(0, 256, (16, 16), np.uint8), g.integers(0, 256, (8, 8), np.uint8), g.integers(0, 256, (8, 8), np.uint8))
        planes = {(s, k): hip.read_frame(s, k) for s in range(2) for k in range(2)}
        n = 70000
        which = (np.arange(n) * 7 + np.arange(n) // 65535) % 4              # (stream, slot) = (which >> 1, which & 1); the pattern shifts at the seam
        dst = DeviceBuffer(lib, n * 24 + TAIL)
        hip.export_resized((which >> 1).tolist(), (which & 1).tolist(), (4, 4), "nv12", out=(dst.ptr, n * 24))
        got = dst.host()
        dst.free()
        four = np.stack([R.expected([planes[(w >> 1, w & 1)]], "nv12", (0, 0, 16, 16), (4, 4)) for w in range(4)])
        assert np.array_equal(got[:n * 24].reshape(n, 24), four[which])
        assert np.all(got[n * 24:] == 0xA5)


TORCH_CHILD = r"""
import sys
import torch                                   # first: the library then shares torch's HIP runtime
if not torch.cuda.is_available():
    print("no device")
    sys.exit(0)
sys.path.insert(0, %r)
import numpy as np
from p264decoder_amd import HipReconstructor
from tests import resize_checker as R
hip = HipReconstructor(5, 3, n_streams=3, slots=2, max_pictures=1)
g = np.random.default_rng(98)
for s in range(3):
    for k in range(2):
        hip.write_frame(s, k, g.integers(0, 256, (48, 80), np.uint8), g.integers(0, 256, (24, 40), np.uint8), g.integers(0, 256, (24, 40), np.uint8))
planes = {(s, k): hip.read_frame(s, k) for s in range(3) for k in range(2)}
streams, slots = [1, 2, 0], [1, 0, 1]
frames = [planes[(s, k)] for s, k in zip(streams, slots)]
size = (34, 18)
mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
scale, bias = [1 / (255 * s) for s in std], [-m / s for m, s in zip(mean, std)]
for fmt, dtype, shape, tdt in (("i420", "u8", (3, 27, 34), torch.uint8), ("nv12", "u8", (3, 27, 34), torch.uint8), ("rgb24", "u8", (3, 18, 34, 3), torch.uint8),
                               ("rgbp", "f32", (3, 3, 18, 34), torch.float32), ("rgbp", "f16", (3, 3, 18, 34), torch.float16), ("rgb24", "f32", (3, 18, 34, 3), torch.float32)):
    sb = (scale, bias) if dtype != "u8" else (None, None)
    out = hip.export_resized(streams, slots, size, fmt, dtype, None, sb[0], sb[1], "bt709")  if fmt.startswith("rgb") else hip.export_resized(streams, slots, size, fmt)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == tdt and tuple(out.shape) == shape, (fmt, out.shape, out.dtype)
    want = R.expected(frames, fmt, (0, 0, 80, 48), size, dtype, sb[0], sb[1], "bt709" if fmt.startswith("rgb") else "bt601")
    assert np.array_equal(out.cpu().numpy().reshape(-1).view(np.uint8), want), (fmt, dtype)
    # an existing tensor is filled in place, here with a window
    per = R.frame_bytes(fmt, 34, 18, dtype)
    mine = torch.full((3, per), 0xA5, dtype=torch.uint8, device="cuda")
    back = hip.export_resized(streams, slots, size, fmt, dtype, (16, 10, 48, 22), sb[0], sb[1], out=mine)
    assert back is mine
    assert np.array_equal(mine.cpu().numpy().reshape(-1), R.expected(frames, fmt, (16, 10, 48, 22), size, dtype, sb[0], sb[1])), fmt
# the documented shape means what it says: channel c of picture i is a normalised plane
out = hip.export_resized(streams, slots, size, "rgbp", "f32", None, 1 / 255, 0.0)
ref = R.expected([frames[1]], "rgbp", (0, 0, 80, 48), size, "f32", 1 / 255, 0.0).view(np.float32).reshape(3, 18, 34)
assert np.array_equal(out[1].cpu().numpy(), ref) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
hip.close()
print("ok")
"""


def test_torch_tensors():
    """out=None returns a tensor of the documented shape and dtype on the device, out= an existing tensor is filled in place.  In a
    process of its own, which imports torch BEFORE the library is loaded (one HIP runtime per process)."""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:          # (looked for, NOT imported: this process keeps the one HIP runtime it has)
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD % root], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if r.returncode == 0 and r.stdout.strip().endswith("no device"):
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]
