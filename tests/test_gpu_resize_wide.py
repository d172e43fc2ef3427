"""p264hip_export_resized where the taps cross strip boundaries and a row has more than one tile.  kernel_resize.h gives a wavefront a
tile of 256 output samples of a row and splits its tile index into (row, column); tests/test_gpu_resize.py's outputs are at most
162 samples wide, so the column is 0 there, and its frame has five strips.  Here: a frame of 19 x 9 macroblocks whose windows reach
all 19 strips or start inside one, to 224 x 224, to 38 x 18 (eight source samples between taps), to 272 x 132, to 400 x 160 (two
luma tile columns, the second part full) and to 516 x 20 (three luma and two chroma tile columns) - and the product's own 120 x 68
with the window 1920 x 1080.  As in test_gpu_resize.py the frames are random planes, the whole destination is prefilled with 0xA5
and ALL of it is compared with tests/resize_checker.py."""
import numpy as np
import pytest

from tests import resize_checker as R
from tests.hip_harness import reconstructor
from tests.test_gpu_export_wide import random_frames
from tests.test_gpu_resize import INSTANCES, SCALES, run, sweep

pytestmark = pytest.mark.gpu

MB_W, MB_H, STREAMS, SLOTS = 19, 9, 2, 2
# (window, output size)
PAIRS = [((0, 0, 304, 144), (224, 224)), ((0, 0, 304, 144), (38, 18)), ((18, 2, 270, 130), (272, 132)), ((130, 66, 174, 78), (400, 160)),
         ((2, 0, 300, 144), (516, 20))]
BATCHES = [([1], [1]), ([1, 0, 1, 1, 0], [1, 0, 1, 1, 1]), ([0, 0, 1, 1], [0, 1, 0, 1])]
FULL_HD = (0, 0, 1920, 1080)
TILE_W = 256


@pytest.fixture(scope="module")
def store(lib):
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        yield hip, random_frames(hip, MB_W, MB_H, STREAMS, SLOTS, 2651)


@pytest.fixture(scope="module")
def full_hd(lib):
    """two streams, one picture each"""
    with reconstructor(lib, 120, 68, n_streams=2, slots=1, max_pictures=1) as hip:
        yield hip, random_frames(hip, 120, 68, 2, 1, 2652)


@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_windows_across_strips_and_tiles(store, fmt, dtype):
    """every kernel instance at the five pairs, three times with the rotation one step further: fifteen calls meet every pitch and
    every destination offset"""
    assert any(size[0] > 2 * TILE_W for _, size in PAIRS) and any(TILE_W < size[0] < 2 * TILE_W for _, size in PAIRS)
    assert any(crop[0] % 16 for crop, _ in PAIRS) and all(crop[0] + crop[2] <= MB_W * 16 and crop[1] + crop[3] <= MB_H * 16 for crop, _ in PAIRS)
    hip, planes = store
    assert sweep(hip, planes, fmt, dtype, PAIRS + PAIRS[1:] + PAIRS[:1] + PAIRS[2:] + PAIRS[:2], BATCHES) == 15


@pytest.mark.parametrize("fmt,dtype,size,offset", [("rgbp", "f32", (224, 224), 0), ("nv12", "u8", (640, 360), 0), ("rgb24", "u8", (226, 226), 1)])
def test_the_full_hd_window(full_hd, fmt, dtype, size, offset):
    """120 x 68 macroblocks, window 1920 x 1080, two pictures at the tight pitch.  224 x 224 planar float32: every lane on the
    16-byte road; 640 x 360 NV12: three luma and two chroma tile columns, the last part full; 226 x 226 RGB24 at an odd address:
    every lane stores its bytes one by one, the last of a row two pixels."""
    hip, planes = full_hd
    scale, bias = SCALES[1] if dtype != "u8" else (None, None)
    assert R.tight_pitch(fmt, size[0], dtype) % 16 == (0 if offset == 0 else 6)
    got, want = run(hip, planes, [1, 0], [0, 0], fmt, FULL_HD, size, dtype, scale, bias, "bt709" if fmt.startswith("rgb") else "bt601", False, 0, 0, offset)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s %s to %s offset %d: %d bytes differ, the first at %d (%d, want %d)" % (fmt, dtype, size, offset, bad.size, bad[0], got[bad[0]], want[bad[0]])
