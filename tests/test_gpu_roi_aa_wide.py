"""p264hip_export_rois_aa where a picture has several tiles, the source span of a tile is wide and the ROIs of one call use tiles of
different widths (kernel_roi_aa.h chooses 64, 32, 16 or 8 output samples per ROI).  The fixtures of tests/test_gpu_resize_aa_wide.py:
19 x 9 macroblocks (304 x 144), and the product's own 120 x 68 macroblocks with one picture.  Random planes, the whole destination
prefilled with 0xA5, ALL of it compared with tests/roi_aa_checker.py."""
import ctypes as C

import pytest

from p264decoder_amd import _native as N
from p264decoder_amd import letterbox
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export import TAIL
from tests.test_gpu_resize import SCALES
from tests.test_gpu_resize_aa_wide import full_hd, same, store  # noqa: F401  (the fixtures)

pytestmark = pytest.mark.gpu


def run(hip, planes, rois, size, fmt, dtype="u8", fill=(16, 128, 128), scale=None, bias=None, matrix="bt601"):
    per = R.frame_bytes(fmt, size[0], size[1], dtype)
    total = len(rois) * per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    hip.export_rois_aa(rois, size, fmt, dtype, fill, scale, bias, matrix, out=(dst.ptr, total - TAIL))
    want = KA.expected(rois, planes, size, fmt, dtype, fill, scale, bias, matrix, total=total)
    got = dst.host()
    dst.free()
    return got, want


def tile_width(hip, roi, size):
    r = N.resize_desc("i420", size, (0, 0, 2, 2), None, filter=N.FILTER_BILINEAR_AA)
    row = tuple(roi) + (0, 0, 0, 0) * (len(roi) == 6)
    return hip.lib.p264hip_roi_aa_tile_width(C.byref(N.Roi(*row)), C.byref(r), None, None)


@pytest.mark.parametrize("fmt,dtype", [("nv12", "u8"), ("rgbp", "f32")])
def test_a_wide_span_and_a_window_inside_strips(store, fmt, dtype):
    hip, planes = store
    scale, bias = SCALES[1] if dtype != "u8" else (None, None)
    rois = [(0, 1, 0, 0, 304, 144, 200, 100, 10, 6), (0, 0, 18, 2, 270, 130, 40, 120, 150, 72)]         # 30.4:1 across; a window that begins inside a strip
    got, want = run(hip, planes, rois, (224, 224), fmt, dtype, (235, 16, 240), scale, bias, "bt709" if fmt.startswith("rgb") else "bt601")
    same(got, want, "%s %s 304 x 144 into (224, 224)" % (fmt, dtype))


def test_full_hd_into_224_planar_f32_with_tiles_of_two_widths(full_hd):
    hip, planes = full_hd
    scale, bias = SCALES[1]
    rois = [(0, 0, 0, 0, 1920, 1080), (0, 0, 0, 0, 1920, 1080, 82, 94, 60, 34), (0, 0, 2, 4, 1916, 1072, 0, 48, 224, 126), (0, 0, 600, 300, 200, 120)]
    assert letterbox(1916, 1072, 224, 224)[2:] == (224, 126)
    # 1920 into 60 has 64 taps on both axes and a narrower tile than its neighbours
    assert [tile_width(hip, r, (224, 224)) for r in rois] == [64, 32, 64, 64]
    assert int(KA.taps(1920, 60)[1].max()) == 64 and int(KA.taps(1080, 34)[1].max()) == 64
    got, want = run(hip, planes, rois, (224, 224), "rgbp", "f32", (16, 128, 128), scale, bias, "bt709")
    same(got, want, "1920 x 1080 into (224, 224)")


@pytest.mark.parametrize("fmt,dtype", [("nv12", "u8"), ("rgb24", "u8")])
def test_full_hd_letterboxed_into_640(full_hd, fmt, dtype):
    hip, planes = full_hd
    rect = letterbox(1920, 1080, 640, 640)
    assert rect == (0, 140, 640, 360)
    got, want = run(hip, planes, [(0, 0, 0, 0, 1920, 1080) + rect], (640, 640), fmt, dtype, (16, 128, 128), None, None, "bt709" if fmt.startswith("rgb") else "bt601")
    same(got, want, "1920 x 1080 letterboxed into (640, 640) %s" % fmt)
