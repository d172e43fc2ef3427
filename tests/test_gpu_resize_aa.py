"""p264hip_export_resized with filter = P264HIP_FILTER_BILINEAR_AA on the MI355X: the fixture of tests/test_gpu_resize.py (5 x 3
macroblocks, 3 streams x 2 slots of random planes), the whole destination prefilled with 0xA5 and ALL of it compared, floats as bytes,
with tests/resize_aa_checker.py applied to the read_frame planes.

Windows: the frame; two that begin and end inside strips; one of 2 x 2 samples.  The frames are random, so a tap taken from outside
the window shows.  Output sizes: the window itself (one tap of 32768: the source), half of it where that is even (1, 3, 3, 1 over 8),
34 x 18 (reducing; 17 chroma samples: the last lane of a row holds one), 162 x 98 (enlarging; three tiles of 64 in a row, seven tile
rows), 4 x 2 (24 taps a sample from the frame) and 6 x 70 (reduces on one axis, enlarges on the other); the 2 x 2 window goes to
2 x 2, 6 x 70 and 34 x 18."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import export_checker as X
from tests import resize_aa_checker as A
from tests import resize_checker as R
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export import BATCHES, KINDS, STREAMS, TAIL, WINDOWS as EXPORT_WINDOWS, run as run_export
from tests.test_gpu_resize import ELEM, INSTANCES, RGB_KINDS, SCALES, WINDOWS, store  # noqa: F401  (store: the module's fixture)

pytestmark = pytest.mark.gpu

SIZES = [None, "half", (34, 18), (162, 98), (4, 2), (6, 70)]
SMALL_SIZES = [(2, 2), (6, 70), (34, 18)]                   # of the 2 x 2 window


def cases():
    """(window, output size) of the sweep"""
    out = []
    for crop in WINDOWS:
        for size in SIZES if crop[2:] != (2, 2) else SMALL_SIZES:
            if size is None:
                size = crop[2:]
            elif size == "half":
                if crop[2] % 4 or crop[3] % 4:
                    continue
                size = (crop[2] // 2, crop[3] // 2)
            if (crop, size) not in out:
                out.append((crop, size))
    return out


def run(hip, planes, streams, slots, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0):
    """one antialiased export into a prefilled destination; returns (what the device holds, what the checker says it holds)"""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    total = offset + (len(streams) - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_resized(streams, slots, size, fmt, dtype, crop, scale, bias, matrix, full, pitch, stride, out=(dst.ptr + offset, total - offset - TAIL),
                       filter="bilinear_aa")
    want = A.expected_aa([planes[(s, k)] for s, k in zip(streams, slots)], fmt, crop, size, dtype, scale, bias, matrix, full, pitch, stride, offset, total)
    got = dst.host()
    dst.free()
    return got, want


def sweep(hip, planes, fmt, dtype, pairs, batches):
    """tests/test_gpu_resize.py's sweep with the antialiased filter: every (window, size) once, rotating pitch, destination offset,
    batch, frame stride, matrix / range and scale set"""
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
    assert len(pairs) == 19 and ((0, 0, 80, 48), (40, 24)) in pairs and ((6, 46, 2, 2), (2, 2)) in pairs and ((6, 46, 2, 2), (4, 2)) not in pairs
    # twice, the second time one step further round, as the bilinear sweep does
    assert sweep(hip, planes, fmt, dtype, pairs + pairs[1:] + pairs[:1], BATCHES) == 38


def test_output_size_equal_to_the_window_is_the_plain_export(store):
    """the kinds of tests/test_gpu_export.py at its windows: filter 2 with width x height = the window writes the bytes
    p264hip_export_frames writes"""
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

    def call(r, cap=2 * per):
        return lib.p264hip_export_resized(hip.h, two, two, 2, C.byref(r), ptr, cap)

    def D(size=size, crop=crop, filter="bilinear_aa", **kw):
        return N.resize_desc("rgbp", size, crop, None, "f16", 1 / 255, filter=filter, **kw)
    assert call(D()) == 0
    hip.sync()
    dst.fill(0xA5)
    # a reduction above 32:1 (80 columns into 2; 66 into 2, the first width the limit refuses), an unknown filter, the unassigned
    # one, a destination one byte short with and without a frame stride
    refused = [lambda: call(D(size=(2, 2), crop=(0, 0, 80, 48))), lambda: call(D(size=(2, 18), crop=(0, 0, 66, 30))), lambda: call(D(filter=3)),
               lambda: call(D(filter=1)), lambda: call(D(), cap=2 * per - 1), lambda: call(D(frame_stride=per + 8), cap=2 * per + 7)]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_resized:"), i
    assert call(D(size=(2, 2), crop=(0, 0, 80, 48))) == -1 and b"32:1" in lib.p264hip_last_error()
    hip.sync()
    assert np.all(dst.host() == 0xA5)
    assert call(D()) == 0
    hip.sync()
    assert np.array_equal(dst.host(), A.expected_aa([planes[(0, 0)], planes[(1, 1)]], "rgbp", crop, size, "f16", 1 / 255, None, total=total))
    dst.free()
