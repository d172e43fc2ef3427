"""Intra 8x8 macroblocks without a GPU: the checker (tests/i8x8_checker.py) against vectors worked out on paper, what the stimulus
sets reach (tests/i8x8_stim.py), the rules of the seam on the host roads (include/p264hip.h: P264_MB_I8X8) and the compact format's
round trip."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from tests import i8x8_checker as I8
from tests import i8x8_stim as IS
from tests import inter_stim
from tests import spec_recon
from tests import t8x8_checker as T8

# the samples of the paper vectors: p[-1, y] = 10 (y + 1), p[x, -1] = 100 + 10 x (x = 0 .. 15), p[-1, -1] = 90
LEFT, TOP, TOPRIGHT, CORNER = [10 * (y + 1) for y in range(8)], [100 + 10 * x for x in range(8)], [180 + 10 * x for x in range(8)], 90
# ... filtered, everything available (8.3.2.2.1):
#   p'[0, -1] = (90 + 2*100 + 110 + 2) >> 2 = 100;  p'[x, -1] = 100 + 10 x for x = 1 .. 14 (a ramp is its own filter);
#   p'[15, -1] = (240 + 3*250 + 2) >> 2 = 248;  p'[-1, -1] = (100 + 2*90 + 10 + 2) >> 2 = 73;
#   p'[-1, 0] = (90 + 2*10 + 20 + 2) >> 2 = 33;  p'[-1, y] = 10 (y + 1) for y = 1 .. 6;  p'[-1, 7] = (70 + 3*80 + 2) >> 2 = 78
F_TOP = [100 + 10 * x for x in range(15)] + [248]
F_LEFT = [33, 20, 30, 40, 50, 60, 70, 78]
F_CORNER = 73


def test_the_reference_sample_filter_and_its_end_cases():
    c = I8.Census()
    fl, ft, fc = I8.filter_samples(*I8.reference_samples(LEFT, TOP, TOPRIGHT, CORNER), census=c)
    assert (fl, ft, fc) == (F_LEFT, F_TOP, F_CORNER)
    # no corner: p'[0, -1] = (3*100 + 110 + 2) >> 2 = 103, p'[-1, 0] = (3*10 + 20 + 2) >> 2 = 13, no p'[-1, -1]
    fl, ft, fc = I8.filter_samples(*I8.reference_samples(LEFT, TOP, TOPRIGHT, None), census=c)
    assert (fl, ft, fc) == ([13] + F_LEFT[1:], [103] + F_TOP[1:], None)
    # the corner with the top only: (3*90 + 100 + 2) >> 2 = 93; with the left only: (3*90 + 10 + 2) >> 2 = 70; alone: 90
    assert I8.filter_samples(*I8.reference_samples(None, TOP, TOPRIGHT, CORNER), census=c) == (None, F_TOP, 93)
    assert I8.filter_samples(*I8.reference_samples(LEFT, None, None, CORNER), census=c) == (F_LEFT, None, 70)
    assert I8.filter_samples(*I8.reference_samples(None, None, None, CORNER), census=c) == (None, None, 90)
    # a top-right without a top is nobody's sample
    assert I8.filter_samples(*I8.reference_samples(None, None, TOPRIGHT, None), census=c) == (None, None, None)
    # the top without its top-right: p[8 .. 15, -1] = p[7, -1] = 170; p'[7, -1] = (160 + 2*170 + 170 + 2) >> 2 = 168, 170 from there on
    fl, ft, fc = I8.filter_samples(*I8.reference_samples(LEFT, TOP, None, CORNER), census=c)
    assert ft == F_TOP[:7] + [168] + [170] * 8 and fl == F_LEFT and fc == F_CORNER
    assert set(c.filter) == {"top[0] with corner", "top[0] without corner", "top[15]", "corner with top only", "corner with left only", "corner alone",
                             "corner with both", "left[0] with corner", "left[0] without corner", "left[7]"}


# per mode: {(x, y): sample} from the filtered samples above, each from the formula of its clause
PAPER = {
    0: {(0, 0): 100, (5, 3): 150, (7, 7): 170},
    1: {(0, 0): 33, (5, 3): 40, (7, 7): 78},
    2: {(0, 0): 91, (7, 7): 91},                           # (1080 + 381 + 8) >> 4
    3: {(0, 0): 110, (4, 3): 180, (6, 7): 240, (7, 6): 240, (7, 7): 246},      # (230 + 2*240 + 248 + 2) >> 2 = 240; (240 + 3*248 + 2) >> 2 = 246
    4: {(1, 0): 96, (2, 0): 110, (7, 0): 160, (0, 0): 70, (3, 3): 70, (0, 1): 40, (0, 2): 26, (0, 3): 30, (0, 7): 70},
    5: {(0, 0): 87, (1, 0): 105, (1, 1): 96, (0, 1): 70, (0, 2): 40, (0, 7): 60},
    6: {(0, 0): 53, (1, 0): 70, (2, 0): 96, (0, 1): 27, (1, 1): 40, (7, 0): 150},
    7: {(0, 0): 105, (0, 1): 110, (7, 7): 210, (7, 6): 205},
    8: {(0, 0): 27, (1, 0): 26, (1, 6): 76, (2, 6): 78, (0, 6): 74, (7, 7): 78, (5, 3): 70},
}


@pytest.mark.parametrize("mode", range(9))
def test_one_block_per_mode_on_paper(mode):
    o = I8.pred8x8(mode, F_LEFT, F_TOP, F_CORNER)
    for (x, y), v in PAPER[mode].items():
        assert int(o[y, x]) == v, (mode, x, y, int(o[y, x]), v)


def test_dc_fall_backs_and_what_a_mode_may_not_read():
    assert int(I8.pred8x8(2, F_LEFT, None, None)[0, 0]) == 48          # (381 + 4) >> 3
    assert int(I8.pred8x8(2, None, F_TOP, None)[3, 3]) == 135          # (1080 + 4) >> 3
    assert int(I8.pred8x8(2, None, None, None)[7, 0]) == 128
    for mode in range(9):
        need = I8.needs(mode)
        for have in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
            args = (F_LEFT if have[0] else None, F_TOP if have[1] else None, F_CORNER if have[2] else None)
            if all(h or not n for n, h in zip(need, have)):
                I8.pred8x8(mode, *args)
            else:
                with pytest.raises(ValueError):
                    I8.pred8x8(mode, *args)
    # the table of include/p264hip.h / 6.4.11.2: block 3 never has a top-right, block 1's corner is the macroblock's top
    assert I8.block_availability(3, 1, 1, 1, 1) == (True, True, True, False)
    assert I8.block_availability(1, 0, 1, 0, 0) == (True, True, True, False) and I8.block_availability(2, 1, 0, 0, 0) == (True, True, True, True)
    assert I8.block_availability(0, 1, 1, 0, 0) == (True, True, False, True)


@pytest.fixture(scope="module")
def sets():
    return {which: getattr(IS, which)() for which in IS.SETS}


def recon(st, cls=I8.SpecRecon):
    spec = cls(st.pic.mb_w, st.pic.mb_h, 3)
    for slot, f in st.frames.items():
        spec.store.write(slot, f)
    return spec, [p.copy() for p in spec.reconstruct(st.pic)]


@pytest.mark.parametrize("which", IS.SETS)
def test_the_sets_reach_what_they_are_there_for(sets, which):
    IS.assert_covered(which, sets[which])


def test_the_census_is_complete(sets):
    """the dense picture through the checker: every legal (mode, block, availability), every case of the filter, every DC case"""
    spec, _ = recon(sets["dense_set"][0])
    assert set(spec.census8.blocks) == IS.all_cases() and len(IS.all_cases()) == 77
    assert len(spec.census8.filter) == 10 and set(spec.census8.dc) == {"both", "left", "top", "none"}
    assert spec.met == 1 and spec.tells["v"] >= 50 and spec.tells["h"] >= 50, spec.tells
    tells = {}
    for st in sets["inter_set"]:
        spec, _ = recon(st)
        assert spec.met == 1
        for k, v in spec.tells.items():
            tells[k] = tells.get(k, 0) + v
    assert tells.get("v", 0) >= 50 and tells.get("h", 0) >= 50, tells


def test_without_a_flag_it_is_the_checker_below():
    stims = inter_stim.b_set()[:1] + inter_stim.residual_set()[:1]
    for st in stims:
        (_, a), (_, b) = recon(st, spec_recon.SpecRecon), recon(st)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), st.name
    from tests import t8x8_stim
    st = t8x8_stim.directed_set()[4]
    (_, a), (_, b) = recon(st, T8.SpecRecon), recon(st)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), st.name


# ---- the seam, host roads -----------------------------------------------------------------------------------------------------
def _pack_roads(lib, pic):
    """return codes of the host-checked roads for the picture: pack_input, pack_compact, records_check_pic"""
    lay = N.InputLayout()
    assert lib.p264hip_input_layout(C.byref(pic.desc), C.byref(lay)) == 0
    buf = np.zeros(lay.bytes, np.uint8)
    a = lib.p264hip_pack_input(C.byref(pic.desc), buf.ctypes.data, buf.size)
    comp = np.zeros(lib.p264hip_compact_bound(C.byref(pic.desc)), np.uint8)
    b = lib.p264hip_pack_compact(C.byref(pic.desc), comp.ctypes.data, comp.size)
    c = lib.p264hip_records_check_pic(C.byref(pic.desc), pic.desc.mb)
    return a, b, c


def test_the_host_roads_refuse_what_the_seam_forbids(lib, sets):
    st = next(s for s in sets["inter_set"] if s.name == "P cluster")
    pic, rec = st.pic, st.pic.mb_records()
    assert int(pic.desc.transform_8x8) == 3
    fl = np.flatnonzero((rec["intra_modes"] & N.MB_I8X8) != 0)
    coded = next(int(m) for m in fl if rec["coef_mask"][m] & 0xffff)
    inter = int(np.flatnonzero(rec["mb_type"] > N.MB_IPCM)[0])
    a, b, c = _pack_roads(lib, pic)
    assert a > 0 and b > 0 and c == -1
    good = HipReconstructor.pack_compact(pic, lib)
    hdr = N.CompactHdr.from_buffer_copy(good[:128].tobytes())
    assert lib.p264hip_compact_check(C.byref(pic.desc), good.ctypes.data, good.size) == 0

    def refused(m, field, value, desc_t8=3, bare=True):
        """bare: p264hip_records_check, which sees no descriptor, refuses the record too"""
        keep, keep_t8 = rec[field][m], pic.desc.transform_8x8
        rec[field][m], pic.desc.transform_8x8 = value, desc_t8
        bad = good.copy()
        bad[hdr.off_rec + 16 * m:hdr.off_rec + 16 * m + 16] = np.frombuffer(rec[m:m + 1].tobytes(), np.uint8)
        try:
            a, b, c = _pack_roads(lib, pic)
            assert a == -1 and b == -1 and c == m, (field, value, desc_t8, a, b, c)
            assert lib.p264hip_compact_check(C.byref(pic.desc), bad.ctypes.data, bad.size) == -1, (field, value)
            assert (lib.p264hip_records_check(pic.desc.mb, pic.n_mb, pic.desc.n_coef_blocks) == m) == bare
        finally:
            rec[field][m], pic.desc.transform_8x8 = keep, keep_t8
    mask = int(rec["coef_mask"][coded])
    k = next(k for k in range(4) if mask >> (4 * k) & 1)
    refused(inter, "intra_modes", int(rec["intra_modes"][inter]) & ~N.MB_T8X8 | N.MB_I8X8)     # not I4x4: an inter record
    i16 = np.flatnonzero(rec["mb_type"] == N.MB_I16x16)
    if len(i16):
        refused(int(i16[0]), "intra_modes", int(rec["intra_modes"][i16[0]]) | N.MB_I8X8)       # ... an Intra16x16 record
    refused(coded, "coef_mask", mask & ~(1 << (4 * k + 2)))                                    # a nibble of 0xB
    refused(coded, "coef_mask", mask & ~(7 << (4 * k)))                                        # ... of 0x8
    refused(coded, "intra_modes", int(rec["intra_modes"][coded]) | N.MB_T8X8)                  # together with MB_T8X8
    for t8 in (0, 1):                                                                          # the descriptor lacks bit 1
        first = int(fl[0]) if t8 else int(np.flatnonzero((rec["intra_modes"] & (N.MB_I8X8 | N.MB_T8X8)) != 0)[0])
        refused(first, "qp", int(rec["qp"][first]), desc_t8=t8, bare=False)
    # ... and bit 1 alone does not admit MB_T8X8 on inter records
    first = int(np.flatnonzero((rec["intra_modes"] & N.MB_T8X8) != 0)[0])
    refused(first, "qp", int(rec["qp"][first]), desc_t8=2, bare=False)
    a, b, c = _pack_roads(lib, pic)
    assert a > 0 and b > 0 and c == -1


def test_pack_and_compact_round_trips(lib, sets):
    for st in sets["dense_set"] + sets["inter_set"]:
        p = st.pic
        plain = HipReconstructor.pack(p, lib)
        view = N.Picture()
        assert lib.p264hip_unpack_input(C.byref(p.desc), plain.ctypes.data, plain.size, C.byref(view)) == 0
        assert view.transform_8x8 == p.desc.transform_8x8 and view.transform_8x8 & N.T8X8_INTRA
        comp = HipReconstructor.pack_compact(p, lib)
        back = HipReconstructor.expand_compact(p, comp, lib)
        lay = N.InputLayout()
        lib.p264hip_input_layout(C.byref(p.desc), C.byref(lay))
        n, nb = p.n_mb, p.desc.n_coef_blocks
        for off, size in ((0, n * 16), (lay.off_mv, n * 64), (lay.off_ref, n * 4), (lay.off_i4, n * 16), (lay.off_coef, nb * 32)):
            assert np.array_equal(back[off:off + size], plain[off:off + size]), (st.name, off)
        assert np.array_equal(back, plain), st.name         # expand(pack_compact(p)) == pack_input(p), byte for byte


def test_abi_mirror_of_the_new_fields(lib):
    assert N.MB_I8X8 == 0x08 and N.T8X8_INTRA == 2
    assert N.LaunchInfo.intra_i8.offset == 60 and C.sizeof(N.LaunchInfo) == 64
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "p264hip.h"\nint main(void) { printf("%zu %zu %d %d", offsetof(p264hip_launch_info_t, intra_i8), sizeof(p264hip_launch_info_t), P264_MB_I8X8, P264_T8X8_INTRA); return 0; }\n'
    import os
    import subprocess
    import tempfile
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I" + inc, os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        out = subprocess.run([os.path.join(td, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out.split() == ["60", "64", "8", "2"]
