"""The host side of the device export (include/p264hip.h: p264hip_export_t), no GPU: the layout and the refusals of
p264hip_export_frame_bytes / p264hip_export_check, the coefficient table and the fixed-point arithmetic against float64, the display
window p264parse_crop reports, the stream writer's --crop option, and the kernels in the code object."""
import ctypes as C
import hashlib
from fractions import Fraction

import numpy as np
import pytest

from p264decoder_amd import _native as N
from p264decoder_amd.recon import Parser
from tests import export_checker as X
from tests import synth_cases

EINVAL = -1
# the table of include/p264hip.h: (cy, R.cv, G.cu, G.cv, B.cu)
TABLE = {("bt601", False): (9539, 13075, -3209, -6660, 16525), ("bt601", True): (8192, 11485, -2819, -5850, 14516),
         ("bt709", False): (9539, 14686, -1747, -4366, 17305), ("bt709", True): (8192, 12901, -1535, -3835, 15201)}


def desc(fmt="i420", crop=(0, 0, 80, 48), **kw):
    return N.export_desc(fmt, crop, None, **kw)


@pytest.mark.parametrize("fmt", X.FORMATS)
def test_frame_bytes_is_the_layout_table(lib, fmt):
    for w, h in ((80, 48), (62, 30), (2, 2), (1920, 1080)):
        tight = 3 * w if fmt == "rgb24" else w
        for pitch in (0, tight, tight + 16, tight + 2):
            p = pitch or tight
            want = {"i420": p * h * 3 // 2, "nv12": p * h * 3 // 2, "rgb24": p * h, "rgbp": 3 * p * h}[fmt]
            e = desc(fmt, (0, 0, w, h), pitch=pitch)
            assert lib.p264hip_export_frame_bytes(C.byref(e)) == want == X.frame_bytes(fmt, w, h, pitch)
            assert lib.p264hip_export_check(C.byref(e), 120, 68) == 0
            for stride, ok in ((want, True), (want + 7, True), (want - 1, False)):
                e.frame_stride = stride
                assert (lib.p264hip_export_check(C.byref(e), 120, 68) == 0) == ok


def test_the_refusals(lib):
    fb, chk = lib.p264hip_export_frame_bytes, lambda e: lib.p264hip_export_check(C.byref(e), 5, 3)
    assert fb(None) == EINVAL and lib.p264hip_export_check(None, 5, 3) == EINVAL
    assert chk(desc()) == 0
    bad = [desc(fmt=4), desc(fmt=-1), desc("rgb24", matrix=2), desc("rgbp", matrix=-1),
           desc("i420", matrix="bt709"), desc("nv12", full_range=True), desc("rgb24", full_range=2),
           desc(crop=(1, 0, 62, 30)), desc(crop=(0, 1, 62, 30)), desc(crop=(0, 0, 61, 30)), desc(crop=(0, 0, 62, 29)),
           desc(crop=(0, 0, 0, 30)), desc(crop=(0, 0, 62, 0)), desc(crop=(-2, 0, 62, 30)), desc(crop=(0, -2, 62, 30)), desc(crop=(0, 0, -2, 30)),
           desc(pitch=78), desc("rgb24", pitch=238), desc("i420", pitch=81), desc("rgbp", pitch=-80)]
    for e in bad:
        assert fb(C.byref(e)) == EINVAL and chk(e) == EINVAL, (e.format, e.matrix, e.full_range, e.crop_left, e.crop_top, e.width, e.height, e.pitch)
    # an odd pitch is I420's alone
    for fmt in ("nv12", "rgbp"):
        assert fb(C.byref(desc(fmt, pitch=81))) > 0
    # the frame: 5 x 3 macroblocks = 80 x 48
    for crop in ((0, 0, 82, 48), (0, 0, 80, 50), (2, 0, 80, 48), (0, 2, 80, 48), (80, 0, 2, 2), (0, 48, 2, 2)):
        e = desc(crop=crop)
        assert fb(C.byref(e)) > 0 and chk(e) == EINVAL, crop
    assert chk(desc(crop=(78, 46, 2, 2))) == 0
    for mb in ((0, 3), (5, 0), (-1, 3)):
        assert lib.p264hip_export_check(C.byref(desc(crop=(0, 0, 2, 2))), *mb) == EINVAL
    e = desc(frame_stride=80 * 48 * 3 // 2 - 1)
    assert fb(C.byref(e)) > 0 and chk(e) == EINVAL
    e.frame_stride = -8
    assert chk(e) == EINVAL


def test_the_coefficient_table_follows_from_the_rationals():
    for (matrix, full), want in TABLE.items():
        kr, kb = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}[matrix]
        kg = 1 - kr - kb
        sy, s = (Fraction(1), Fraction(1)) if full else (Fraction(255, 219), Fraction(255, 224))
        exact = (sy, 2 * (1 - kr) * s, -2 * kb * (1 - kb) * s / kg, -2 * kr * (1 - kr) * s / kg, 2 * (1 - kb) * s)
        got = tuple((c * 8192 + Fraction(1, 2)).numerator // (c * 8192 + Fraction(1, 2)).denominator for c in exact)      # floor, also of negatives
        assert got == want == X.coefficients(matrix, full), (matrix, full)


@pytest.mark.parametrize("matrix,full", sorted(TABLE))
def test_the_arithmetic_is_within_1_of_float64(matrix, full):
    g = np.random.default_rng(264)
    t = g.integers(0, 256, size=(3, 200000))
    edge = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255])
    lines = np.arange(256)
    corners = np.stack(np.meshgrid(edge, edge, edge, indexing="ij")).reshape(3, -1)
    # the twelve edges of the cube: one coordinate runs, the other two sit in corners
    edges = [np.roll(np.array([lines, np.full(256, a), np.full(256, b)]), k, axis=0) for k in range(3) for a in (0, 255) for b in (0, 255)]
    for y, cb, cr in [t, corners] + edges:
        fixed, peak = X.rgb(y, cb, cr, matrix, full)
        real = X.rgb_real(y, cb, cr, matrix, full)
        assert peak < 1 << 23
        for f, r in zip(fixed, real):
            assert int(np.abs(f.astype(np.int64) - r).max()) <= 1


def crop_of(args, n_pictures=1):
    ps = Parser()
    before = ps.crop
    pics = ps.parse_stream(open(synth_cases.generate(args), "rb").read(), limit=n_pictures)
    assert len(pics) == n_pictures
    return before, ps.crop, (pics[0].mb_w, pics[0].mb_h)


def test_parse_crop(lib):
    small = "--frames 1 --seed 5 --coded 10 --maxlevel 4"
    before, crop, mb = crop_of("--mbw 120 --mbh 68 --crop-bottom 4 " + small)
    assert before is None and crop == (0, 0, 1920, 1080) and mb == (120, 68)          # (what the parser delivers stays MB-aligned)
    assert crop_of("--mbw 8 --mbh 6 --crop 1 2 3 1 " + small)[1] == (2, 6, 122, 88)
    assert crop_of("--mbw 8 --mbh 6 " + small)[1] == (0, 0, 128, 96)
    assert crop_of("--mbw 8 --mbh 6 --crop 0 0 0 0 " + small)[1] == (0, 0, 128, 96)
    # offsets that leave no sample: no window
    assert crop_of("--mbw 2 --mbh 2 --crop 8 8 0 0 " + small)[1] is None
    assert crop_of("--mbw 2 --mbh 2 --crop 0 0 0 16 " + small)[1] is None
    assert lib.p264parse_crop(None, None, None, None, None) == -1
    # null outputs are skipped
    ps = Parser()
    ps.parse_stream(open(synth_cases.generate("--mbw 8 --mbh 6 --crop 1 2 3 1 " + small), "rb").read(), limit=1)
    w = C.c_int()
    assert lib.p264parse_crop(ps.h, None, None, C.byref(w), None) == 0 and w.value == 122


def test_streams_without_the_crop_option_are_the_bytes_of_before():
    for name in ("cif_ip", "qpd_1080p"):                    # without cropping, and with --crop-bottom
        assert hashlib.sha256(synth_cases.stream_bytes(name)).hexdigest() == synth_cases.golden(name)[0], name
    # --crop 0 0 0 B writes what --crop-bottom B writes
    a = "--mbw 8 --mbh 6 --frames 2 --seed 9 --coded 10 --maxlevel 4 "
    assert open(synth_cases.generate(a + "--crop 0 0 0 3"), "rb").read() == open(synth_cases.generate(a + "--crop-bottom 3"), "rb").read()


def test_the_kernels_are_in_the_code_object_without_spills_or_scratch(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    for k in ("k_export_i420", "k_export_nv12", "k_export_rgb24", "k_export_rgbp"):
        assert k in res, sorted(res)
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)


def test_the_wide_windows_reach_every_tile_column():
    """the windows of tests/test_gpu_export_wide.py: three luma tile columns, two I420 chroma tile columns, the odd last strip pair,
    a window whose first strip is no multiple of the tile - restated from the windows and held against the table that file keeps"""
    from tests import test_gpu_export_wide as W
    W.assert_reach()
    assert len(W.WINDOWS) == 6 and {r[2] for r in W.WINDOWS.values()} == {2, 3} and {r[5] for r in W.WINDOWS.values()} == {1, 2}
    assert any(r[0] % 8 for r in W.WINDOWS.values()) and any(c[0] % 16 for c in W.WINDOWS)
    assert {fmt for fmt, _, _ in W.KINDS} == set(X.FORMATS) and len(W.KINDS) == 10


def test_abi_mirror(lib):
    import os
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "p264pipe.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(p264hip_export_t), offsetof(p264hip_export_t, pitch), offsetof(p264hip_export_t, frame_stride)); return 0; }\n'
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I" + inc, os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(td, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(N.Export), N.Export.pitch.offset, N.Export.frame_stride.offset] == [40, 28, 32]
    for f in ("p264hip_export_frames", "p264parse_crop", "p264pipe_crop", "p264pipe_export_last", "p264pipe_set_sink"):
        assert hasattr(lib, f)
