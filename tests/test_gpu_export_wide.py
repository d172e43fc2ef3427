"""p264hip_export_frames beyond one tile column.  kernel_export.h walks a picture in tiles of 8 strips x 32 rows and a wavefront
splits its tile index into (ty, tx); tests/test_gpu_export.py's frame of 5 x 3 macroblocks has one tile column in every format, so
tx is 0 there.  Here: a frame of 19 x 9 macroblocks - 19 strips are luma (and NV12) tile columns of 8 + 8 + 3, its 10 strip pairs are
I420 chroma tile columns of 8 + 2 with one strip in the last pair, 18 row groups are five tile rows with the last half full - and the
product's own 120 x 68 with the window 1920 x 1080 (15 x 34 luma tiles, 8 I420 chroma tile columns).  As in test_gpu_export.py the
frames are random planes put there with write_frame, the whole destination is prefilled with 0xA5 and ALL of it is compared with
tests/export_checker.py.

WINDOWS says per window what it reaches; `reach` restates the tile counts from the window alone and every test asserts the two
agree, so that a change of windows cannot quietly shrink the coverage to one column again (tests/test_export_cpu.py asserts it
without a device)."""
import numpy as np
import pytest

from tests import export_checker as X
from tests.hip_harness import reconstructor
from tests.test_gpu_export import KINDS, run

pytestmark = pytest.mark.gpu

MB_W, MB_H, STREAMS, SLOTS = 19, 9, 2, 2
# window (x0, y0, w, h): (first strip, strips, luma tile columns, luma tile rows, I420 strip pairs, I420 chroma tile columns, NV12 chroma tile columns)
WINDOWS = {
    (0, 0, 304, 144): (0, 19, 3, 5, 10, 2, 3),       # the whole frame: 16-byte luma stores in every column, the odd last pair
    (0, 0, 288, 144): (0, 18, 3, 5, 9, 2, 3),        # chroma width 144: I420's 16-byte path in a second chroma column
    (16, 8, 272, 128): (1, 17, 3, 4, 9, 2, 3),       # strip-aligned luma whose I420 pairs start mid-pair
    (130, 66, 174, 78): (8, 11, 2, 3, 6, 1, 2),      # begins inside strip 8, below the first tile row, ends at the frame's edge
    (2, 2, 300, 140): (0, 19, 3, 5, 10, 2, 3),       # every strip touched, nothing aligned
    (160, 0, 144, 144): (10, 9, 2, 5, 5, 1, 2),      # s0 = 10, c0 = 5: tile columns count from the window, not from the frame
}
# (streams, slots) of a call: one picture; five with a repeated entry and out of order; all four frames
BATCHES = [([1], [1]), ([1, 0, 1, 1, 0], [1, 0, 1, 1, 1]), ([0, 0, 1, 1], [0, 1, 0, 1])]
FULL_HD = (0, 0, 1920, 1080)


def reach(crop):
    """the tile counts of a window, from include/p264hip.h's layout and kernel_export.h's tile shape (8 strips of 16 samples x 4
    groups of 8 rows; I420 chroma: 8 strip PAIRS), in the order of WINDOWS' values"""
    x0, y0, w, h = crop
    s0, s1 = x0 // 16, (x0 + w - 1) // 16
    n_cols = s1 - s0 + 1
    n_groups = (y0 + h - 1) // 8 - y0 // 8 + 1
    pairs = s1 // 2 - s0 // 2 + 1
    return s0, n_cols, -(-n_cols // 8), -(-n_groups // 4), pairs, -(-pairs // 8), -(-n_cols // 8)


def assert_reach():
    for crop, want in WINDOWS.items():
        assert reach(crop) == want, (crop, reach(crop), want)
        assert crop[0] + crop[2] <= MB_W * 16 and crop[1] + crop[3] <= MB_H * 16
    three = [c for c, r in WINDOWS.items() if r[2] == 3 and r[5] == 2]
    assert len(three) >= 4 and any(r[4] == 10 for r in WINDOWS.values())       # (10 pairs of 19 strips: the last pair has one strip)
    assert reach(FULL_HD) == (0, 120, 15, 34, 60, 8, 15)


def random_frames(hip, mb_w, mb_h, streams, slots, seed):
    g = np.random.default_rng(seed)
    w, h = mb_w * 16, mb_h * 16
    for s in range(streams):
        for k in range(slots):
            # (full range of every plane: the RGB clips are reached)
            hip.write_frame(s, k, g.integers(0, 256, (h, w), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8), g.integers(0, 256, (h // 2, w // 2), np.uint8))
    return {(s, k): hip.read_frame(s, k) for s in range(streams) for k in range(slots)}


@pytest.fixture(scope="module")
def store(lib):
    """a context of 19 x 9 macroblocks whose four frames hold random planes, and those planes as read_frame returns them"""
    with reconstructor(lib, MB_W, MB_H, n_streams=STREAMS, slots=SLOTS, max_pictures=STREAMS) as hip:
        yield hip, random_frames(hip, MB_W, MB_H, STREAMS, SLOTS, 2641)


@pytest.fixture(scope="module")
def full_hd(lib):
    with reconstructor(lib, 120, 68, n_streams=1, slots=2, max_pictures=1) as hip:
        yield hip, random_frames(hip, 120, 68, 1, 2, 2642)


@pytest.mark.parametrize("fmt,matrix,full", KINDS)
def test_every_window_in_every_tile_column(store, fmt, matrix, full):
    """every window of WINDOWS (each format and each RGB matrix / range meets all six) at the pitches tight, tight + 16 and tight + 2
    and the destination offsets 0, 1 and 4; one picture, five with a repeated entry and all four, with and without a frame_stride"""
    assert_reach()
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


@pytest.mark.parametrize("fmt,offset", [("i420", 0), ("nv12", 0), ("rgb24", 0), ("rgbp", 0), ("nv12", 1), ("rgb24", 1)])
def test_the_full_hd_window(full_hd, fmt, offset):
    """120 x 68 macroblocks, window 1920 x 1080, two pictures at the tight pitch: 15 x 34 luma tiles and 8 I420 chroma tile columns of
    full pairs exist at no smaller size.  Offset 0: every lane stores 16 bytes at a time; offset 1: the byte path."""
    assert_reach()
    hip, planes = full_hd
    assert X.frame_bytes(fmt, 1920, 1080) % 16 == 0
    got, want = run(hip, planes, [0, 0], [1, 0], fmt, FULL_HD, "bt709" if fmt.startswith("rgb") else "bt601", False, 0, 0, offset)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s offset %d: %d bytes differ, the first at %d (%d, want %d)" % (fmt, offset, bad.size, bad[0], got[bad[0]], want[bad[0]])
