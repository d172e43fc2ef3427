"""The antialiased resized export where a picture has several tiles and the source span of a tile is wide.  kernel_resize_aa.h gives
a workgroup a tile of TW = 64 by TH = 16 luma samples (the host halves TW, down to 8, until the tile's source columns fit the LDS).
A frame of 19 x 9 macroblocks (304 x 144, tests/test_gpu_export_wide.py's), one stream x 2 slots, to 34 x 18, 10 x 6 (30.4 : 1 across:
one tile spans all 19 strips), 224 x 224, 150 x 72, to the widths 2 TW - 2, 2 TW and 2 TW + 2 and the heights TH - 2 and TH + 2; and the product's own
120 x 68 macroblocks with the window 1920 x 1080 to 224 x 224 planar float32 with the ImageNet scale and bias, to 640 x 360 NV12 and
to 60 x 34 I420 - 64 taps on both axes (32 : 1 and 31.8 : 1), the widest tile span (TW = 32: 65 luma and 66 chroma strips) - and a window that begins
and ends inside strips.  Random planes, the whole destination prefilled with 0xA5, ALL of it compared with
tests/resize_aa_checker.py."""
import numpy as np
import pytest

from tests.hip_harness import reconstructor
from tests.test_gpu_export_wide import random_frames
from tests.test_gpu_resize import SCALES
from tests.test_gpu_resize_aa import run

pytestmark = pytest.mark.gpu

MB_W, MB_H = 19, 9
FRAME = (0, 0, 304, 144)
TW, TH = 64, 16
SIZES = [(34, 18), (10, 6), (224, 224), (150, 72), (2 * TW - 2, TH - 2), (2 * TW, TH + 2), (2 * TW + 2, TH - 2), (TW - 2, TH + 2), (TW + 2, 2 * TH)]
FORMATS = [("nv12", "u8"), ("i420", "u8"), ("rgbp", "f32"), ("rgb24", "f16")]
FULL_HD = (0, 0, 1920, 1080)


@pytest.fixture(scope="module")
def store(lib):
    with reconstructor(lib, MB_W, MB_H, n_streams=1, slots=2, max_pictures=1) as hip:
        yield hip, random_frames(hip, MB_W, MB_H, 1, 2, 2661)


@pytest.fixture(scope="module")
def full_hd(lib):
    """one stream, one picture"""
    with reconstructor(lib, 120, 68, n_streams=1, slots=1, max_pictures=1) as hip:
        yield hip, random_frames(hip, 120, 68, 1, 1, 2662)


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d bytes differ, the first at %d (%d, want %d)" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("fmt,dtype", FORMATS)
def test_several_tiles_and_their_edges(store, fmt, dtype):
    hip, planes = store
    scale, bias = SCALES[1] if dtype != "u8" else (None, None)
    for n, size in enumerate(SIZES):
        crop = FRAME if n % 3 else (18, 2, 270, 130)        # (every third from a window that begins inside a strip)
        streams, slots = ([0, 0], [1, 0]) if n % 2 else ([0], [1])
        got, want = run(hip, planes, streams, slots, fmt, crop, size, dtype, scale, bias, "bt709" if fmt.startswith("rgb") else "bt601", bool(n & 1) and fmt.startswith("rgb"),
                        0, 0, (0, 4)[n % 2])
        same(got, want, "%s %s %s to %s" % (fmt, dtype, crop, size))


@pytest.mark.parametrize("fmt,dtype,crop,size", [("rgbp", "f32", FULL_HD, (224, 224)), ("nv12", "u8", FULL_HD, (640, 360)), ("i420", "u8", FULL_HD, (60, 34)),
                                                 ("rgbp", "f32", (2, 4, 1916, 1072), (224, 224))])
def test_the_full_hd_window(full_hd, fmt, dtype, crop, size):
    hip, planes = full_hd
    scale, bias = SCALES[1] if dtype != "u8" else (None, None)
    got, want = run(hip, planes, [0], [0], fmt, crop, size, dtype, scale, bias, "bt709" if fmt.startswith("rgb") else "bt601")
    same(got, want, "%s %s %s to %s" % (fmt, dtype, crop, size))
