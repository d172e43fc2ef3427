"""tests/limit_geometry.py on the CPU: every geometry flips the switch it is on the list for and no other it claims not to (the
conditions restated from the headers' constants, which are read out of the headers; the bands of the work lists from the C++ plan
itself); the drawn pictures hold what the GPU file relies on; they are the pictures of tests/golden/limit_geometry.json, and for the
two smallest golden geometries the checker gives the file's hashes; the compact road's limit on the host (the packer, the header
check, the host reference of k_expand_compact at M = 2 and M = 8); the export and resize tables at the far end of the largest frame."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from p264decoder_amd.recon import P264Error
from tests import hip_harness as H
from tests import limit_geometry as L
from tests import scaling_checker as SC
from tests import seam_fuzz
from tests.test_launch_plan_cpu import CU, plan                     # noqa: F401  (plan: that module's fixture, the C++ launch plan)
from tests.test_resize_aa_cpu import host_taps

EINVAL = -1
FRAME_W, FRAME_H = 2047 * 16, 512 * 16


# ---- the table of geometries -------------------------------------------------------------------------------------------------------
def test_the_conditions_are_the_headers(plan):
    """switches() restates three conditions: each stands in its header in these words; the limits of p264hip_create are the entry's
    fields; the work lists' bands are the C++ plan's"""
    c = L.constants()
    text = lambda f: open(os.path.join(L.HIP, f)).read()
    sp = r"\s*"
    cond = lambda *parts: sp.join(re.escape(x) for x in parts)
    assert re.search(cond("keep", "=", "!BPIC", "&&", "g.n_mb", "<=", "MC_SORT_KEEP", "*", "MC_SORT_THREADS", ";"), text("kernel_mc_sort.h"))
    assert re.search(cond("wins", "=", "(", "g.mb_w", "+", "63", ")", "/", "64", ",", "n_win", "=", "g.mb_h", "*", "wins", ";"), text("kernel_intra.h"))
    assert re.search(cond("use_free", "=", "pd->slice_type", "!=", "P264_SLICE_I", "&&", "n_win", "<=", "INTRA_MASKS", "&&", "g.n_mb", "<", "65536", ";"), text("kernel_intra.h"))
    assert re.search(cond("M", "=", "(", "n", "+", "EXPAND_THREADS", "-", "1", ")", "/", "EXPAND_THREADS", ","), text("kernel_expand.h"))
    assert re.search(cond("#define", "MAX_BANDS", "(", "MAX_MB_ROWS", "/", "2", ")"), text("kernel_deblock.h"))
    assert re.search(cond("progress", "[", "MAX_MB_ROWS", "/", "INTRA_BAND", "+", "1", "]"), text("kernel_intra.h"))
    assert re.search(cond("n", ">", "P264HIP_COMPACT_MAX_MB"), open(os.path.join(L.ROOT, "p264decoder_amd", "csrc", "host", "compact.c")).read())
    assert re.search(r"mb_w > MCE_MAX_MB_W \|\| mb_h < 1 \|\| mb_h > MAX_MB_ROWS", text("p264hip.hip"))
    assert c["MC_SORT_KEEP"] * c["MC_SORT_THREADS"] == c["P264HIP_COMPACT_MAX_MB"] == 8192 and c["INTRA_MASKS"] == 160
    assert (1 << c["MCE_COL_BITS"]) - 1 == 2047 and c["MAX_MB_ROWS"] == 512 <= 1 << c["MCE_ROW_BITS"]
    got = plan([g + (1, CU, {"p": True}, {}) for g in L.GEOMETRIES])
    for g, d in zip(L.GEOMETRIES, got):
        sw = L.switches(g)
        assert (d["band_log2"], d["n_bands"]) == (sw["mc_band_log2"], sw["mc_bands"]) and d["n_bands"] <= c["MC_MAX_BANDS"], (g, d)


def test_every_row_flips_the_switch_it_claims():
    c = L.constants()
    sw = {g: L.switches(g) for g in L.GEOMETRIES}
    pick = lambda name: {g: s[name] for g, s in sw.items()}
    # keep: off on 64 x 129 alone; 64 x 128 is the last with it (one more macroblock and it is off)
    assert [g for g, v in pick("keep").items() if not v] == [(64, 129)] and sw[(64, 128)]["n_mb"] == c["MC_SORT_KEEP"] * c["MC_SORT_THREADS"]
    # use_free: off on 1 x 161, 65 x 81 and 3 x 512, by n_win alone (n_mb < 65536 everywhere); 1 x 160 sits on the limit; 64 x 129 keeps it
    assert [g for g, v in pick("use_free").items() if not v] == [(1, 161), (65, 81), (3, 512)]
    assert pick("n_win") == {(1, 160): 160, (1, 161): 161, (65, 81): 162, (64, 128): 128, (64, 129): 129, (33, 32): 32, (3, 512): 512, (2047, 2): 64}
    assert sw[(1, 160)]["n_win"] == c["INTRA_MASKS"] and sw[(64, 129)]["use_free"] and not sw[(64, 129)]["keep"]
    # the compact road: refused on 64 x 129 alone; M and the idle threads of k_expand_compact
    assert [g for g, v in pick("compact").items() if not v] == [(64, 129)]
    assert (sw[(64, 128)]["M"], sw[(64, 128)]["idle"]) == (8, 0) and (sw[(33, 32)]["M"], sw[(33, 32)]["idle"]) == (2, 496)
    assert sw[(1, 160)]["M"] == sw[(1, 161)]["M"] == 1 and sw[(65, 81)]["M"] == 6 and sw[(33, 32)]["n_mb"] % 1024 and sw[(33, 32)]["n_mb"] // 1024 == 1
    # the limits: the last row and every entry of the progress arrays, MC_MAX_BANDS bands without a knob, MAX_BANDS of the loop filter; the last column
    tall, wide = sw[(3, 512)], sw[(2047, 2)]
    assert tall["last_row"] == c["MAX_MB_ROWS"] - 1 and tall["mc_bands"] == c["MC_MAX_BANDS"] and tall["mc_band_log2"] == 4
    assert tall["intra_bands"] == c["MAX_MB_ROWS"] // c["INTRA_BAND"] == 128 and tall["deblock_bands_rb1"] == c["MAX_MB_ROWS"] // 2 == 256
    assert all(s["mc_bands"] < c["MC_MAX_BANDS"] for g, s in sw.items() if g != (3, 512))
    assert wide["last_col"] == (1 << c["MCE_COL_BITS"]) - 2 and wide["n_win"] == 2 * 32
    assert sw[(1, 161)]["intra_bands"] == 41 > c["INTRA_ROW_WAVES"]
    # rows from 256 and columns from 1024 on: the top bit of an entry's fields is set on these two alone
    assert [g for g in L.GEOMETRIES if g[1] > 256] == [(3, 512)] and [g for g in L.GEOMETRIES if g[0] > 1024] == [(2047, 2)]


@pytest.mark.parametrize("geometry", L.GEOMETRIES, ids=L.IDS)
def test_the_drawn_pictures_hold_what_their_names_say(geometry):
    L.assert_covered(geometry, L.main_set(geometry))
    if geometry in L.FAST_GEOMETRIES:
        L.assert_fast_covered(geometry, L.fast_set(geometry))


@pytest.mark.parametrize("geometry", L.LIMIT_GEOMETRIES, ids=L.IDS)
def test_limit_vectors_lie_inside_the_picture(geometry):
    for st in L.limit_vector_set(geometry):
        L.assert_limit_covered(st)
        wp = L.weighted_twin(st)
        assert int(wp.pic.desc.explicit_wp) == 1 and int(st.pic.desc.explicit_wp) == 0 and wp.pic.mv is st.pic.mv


# ---- the golden file ---------------------------------------------------------------------------------------------------------------
def test_the_golden_file_s_pictures_are_the_drawn_ones():
    listed = L.golden_pictures()
    assert sorted(k for k, _, _ in listed) == sorted(L.golden()) and len(listed) == len(L.golden())
    for key, st, checker in listed:
        entry = L.golden()[key]
        assert entry["digest"] == seam_fuzz.picture_digest(st.pic) and entry["checker"] == checker and len(entry["planes"]) == 3, key
    for g in L.SCALED_GEOMETRIES + L.CR_GEOMETRIES:
        for st in ([L.scaled_picture(g)] if g in L.SCALED_GEOMETRIES else []) + ([L.cr_picture(g)] if g in L.CR_GEOMETRIES else []):
            L.assert_intra_covered(g, st.pic)


@pytest.mark.parametrize("geometry", L.HIGH_GEOMETRIES, ids=L.IDS)
def test_the_checker_gives_the_golden_hashes(geometry):
    """the two smallest golden geometries: generator, stimulus and file are one"""
    for i, st in enumerate(L.high_set(geometry)):
        assert not SC.census(st.pic)[1], st.name
        want = L.golden()["%s/high/%d %s" % (L.IDS(geometry), i, st.name)]["planes"]
        assert L.plane_hashes(H.expect(st, SC.SpecRecon, L.SLOTS)) == want, st.name


# ---- the compact road's limit ----------------------------------------------------------------------------------------------------------
def pack_compact_rc(lib, pic):
    buf = np.zeros(lib.p264hip_compact_bound(C.byref(pic.desc)), np.uint8)
    return lib.p264hip_pack_compact(C.byref(pic.desc), buf.ctypes.data, buf.size), buf


def test_the_compact_road_ends_at_8192_macroblocks(lib):
    for kind in ("P", "B implicit"):
        ok, over = L.main_picture((64, 128), kind).pic, L.main_picture((64, 129), kind).pic
        n, blk = pack_compact_rc(lib, ok)
        assert n > 0 and lib.p264hip_compact_header_ok(C.byref(ok.desc), blk.ctypes.data, n) == 1
        hdr = N.CompactHdr.from_buffer_copy(blk[:128].tobytes())
        assert hdr.n_mb == 8192
        assert pack_compact_rc(lib, over)[0] == EINVAL
        with pytest.raises(P264Error):
            HipReconstructor.pack_compact(over, lib)
        # a header that is consistent for its picture, sections laid out as the packer lays them out: accepted at 8192 macroblocks,
        # refused at 8256 - the limit, which keeps k_expand_compact's tables inside LDS, is the only thing that differs
        a, b = L.consistent_header(ok), L.consistent_header(over)
        assert N.CompactHdr.from_buffer_copy(a[:128].tobytes()).n_mb == 8192 and N.CompactHdr.from_buffer_copy(b[:128].tobytes()).n_mb == 8256
        assert lib.p264hip_compact_header_ok(C.byref(ok.desc), a.ctypes.data, a.size) == 1
        assert lib.p264hip_compact_header_ok(C.byref(over.desc), b.ctypes.data, b.size) == 0
        assert lib.p264hip_compact_check(C.byref(over.desc), b.ctypes.data, b.size) == EINVAL


@pytest.mark.parametrize("geometry", [(33, 32), (64, 128)], ids=L.IDS)
def test_the_host_expansion_gives_the_arrays_back(lib, geometry):
    """p264hip_expand_compact, the host reference of k_expand_compact, where a thread owns 2 and 8 macroblocks: every section of the
    slot layout, for one picture of each kind - the High-profile ones with P264_MB_T8X8, Intra 8x8 modes, weights and lists among them"""
    pics = [st.pic for st in L.main_set(geometry).values()]
    pics += [st.pic for st in L.fast_set(geometry).values()]        # T8X8 records, Intra 8x8 modes, off_wp and off_scaling at M > 1
    if geometry == (33, 32):
        pics.append(L.scaled_picture(geometry).pic)
    for p in pics:
        plain, comp = HipReconstructor.pack(p, lib), HipReconstructor.pack_compact(p, lib)
        assert lib.p264hip_compact_check(C.byref(p.desc), comp.ctypes.data, comp.size) == 0 and comp.size < plain.size
        back = HipReconstructor.expand_compact(p, comp, lib)
        lay = N.InputLayout()
        assert lib.p264hip_input_layout(C.byref(p.desc), C.byref(lay)) == 0
        n, nb = p.n_mb, int(p.desc.n_coef_blocks)
        parts = [(lay.off_mb, n * 16), (lay.off_mv, n * 64), (lay.off_ref, n * 4), (lay.off_i4, n * 16), (lay.off_coef, nb * 32)]
        if int(p.desc.slice_type) == N.SLICE_B:
            parts += [(lay.off_mv_l1, n * 64), (lay.off_ref_l1, n * 4), (lay.off_weights, N.MAX_REFS * N.MAX_REFS)]
        if int(p.desc.explicit_wp):
            parts.append((lay.off_wp, 384))
        if int(p.desc.scaling_lists):
            parts.append((lay.off_scaling, N.SCALING_BYTES))
        for off, size in parts:
            assert np.array_equal(back[off:off + size], plain[off:off + size]), (geometry, off, size)


# ---- the export and resize tables at the far end of the largest frame ------------------------------------------------------------------
def test_windows_at_the_far_end_of_the_largest_frame(lib):
    for fmt in ("i420", "nv12", "rgb24", "rgbp"):
        for crop, ok in (((0, 0, FRAME_W, FRAME_H), True), ((FRAME_W - 2, FRAME_H - 2, 2, 2), True), ((32000, 7600, 752, 592), True),
                         ((FRAME_W - 2, 0, 4, 2), False), ((0, FRAME_H - 2, 2, 4), False), ((FRAME_W, 0, 2, 2), False)):
            e = N.export_desc(fmt, crop)
            assert (lib.p264hip_export_check(C.byref(e), 2047, 512) == 0) == ok, (fmt, crop)
            assert lib.p264hip_export_check(C.byref(e), 2047, 2) == (0 if ok and crop[1] + crop[3] <= 32 else EINVAL), (fmt, crop)
            for filt, size in (("bilinear", (94, 74)), ("bilinear_aa", (94, 74))):
                if crop[2] >= 752:
                    r = N.resize_desc(fmt, size if crop[2] == 752 else (16384, 8192), crop, None, filter=filt)
                    assert (lib.p264hip_resize_check(C.byref(r), 2047, 512) == 0) == ok, (fmt, crop, filt)
    r = N.resize_desc("rgbp", (94, 4), (32002, 0, 752, 32), None, filter="bilinear_aa")
    assert lib.p264hip_resize_check(C.byref(r), 2047, 2) == EINVAL and lib.p264hip_resize_check(C.byref(r), 2047, 512) == EINVAL


@pytest.mark.parametrize("S,D", [(FRAME_W, 16384), (FRAME_W, 1024), (FRAME_H, 256), (FRAME_H, 8192), (FRAME_W // 2, 512), (752, 94), (752, 48), (592, 74)])
def test_taps_of_the_longest_axes(lib, S, D):
    """an axis as long as the frame allows: the last first, first + count inside the axis, weights of 32768"""
    pos = (C.c_int32 * D)()
    assert lib.p264hip_resize_taps(S, D, pos) == 0
    p = np.ctypeslib.as_array(pos).astype(np.int64)
    assert p.min() >= 0 and p.max() <= (S - 1) * 256 and np.all(np.diff(p) >= 0) and p[-1] >> 8 >= S - 1 - -(-S // D)
    if S <= 32 * D:
        first, count, w = host_taps(lib, S, D)
        assert first.min() >= 0 and np.all(first + count <= S) and first[-1] + count[-1] == S and np.all(np.diff(first) >= 0)
        assert np.all(w.sum(axis=1) == 32768) and count.min() >= 1 and count.max() <= N.AA_MAX_TAPS
        assert first[-1] >= S - 2 * -(-S // D) - 2 and (S < 8192 or first[-1] > 4095)           # (beyond 12 bits on the long axes)
        assert first.max() | (int(count.max()) << 16) < 1 << 32
