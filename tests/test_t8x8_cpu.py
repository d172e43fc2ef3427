"""The 8x8 transform of inter macroblocks without a GPU: the checker (tests/t8x8_checker.py) against itself and against
tests/spec_recon.py where no record carries the flag, what the stimulus sets reach (tests/t8x8_stim.py), the rules of the seam on
the host roads (include/p264hip.h: P264_MB_T8X8) and the kernel in the code object."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from tests import inter_stim
from tests import residual_checker as RC
from tests import spec_recon
from tests import t8x8_checker as T8
from tests import t8x8_stim as TS

# the basis of the one-dimensional stage, row k = what input k contributes to the eight outputs, times 8
BASIS = [[8, 8, 8, 8, 8, 8, 8, 8], [12, 10, 6, 3, -3, -6, -10, -12], [8, 4, -4, -8, -8, -4, 4, 8], [10, -3, -12, -6, 6, 12, 3, -10],
         [8, -8, -8, 8, 8, -8, -8, 8], [6, -12, 3, 10, -10, -3, 12, -6], [4, -8, 8, -4, -4, 8, -8, 4], [3, -6, 10, -12, 12, -10, 6, -3]]


def test_the_stage_is_the_orthogonal_8_12_10_6_3_8_4_basis():
    m = [T8.stage([8 if i == k else 0 for i in range(8)]) for k in range(8)]          # (inputs of 8: no shift of the stage truncates)
    assert m == BASIS
    for i in range(8):
        for j in range(i):
            assert sum(a * b for a, b in zip(m[i], m[j])) == 0, (i, j)


def test_dc_only_and_single_coefficient_blocks():
    for qp in (0, 17, 35, 36, 51):
        lv = [0] * 64
        lv[0] = 3
        r = T8.block8x8(lv, qp, RC.Range())
        d = T8.scale8x8(T8.unscan8(lv), qp, RC.Range())[0][0]
        assert d != 0 and all(x == (d + 32) >> 6 for row in r for x in row), qp
    rng = RC.Range()
    for u in range(8):
        for v in range(8):
            d = [[0] * 8 for _ in range(8)]
            d[u][v] = 512                                                          # (every shift of both stages exact)
            r = T8.transform8x8(d, rng)
            assert r == [[(8 * BASIS[u][i] * BASIS[v][j] + 32) >> 6 for j in range(8)] for i in range(8)], (u, v)
    assert rng.ok and rng.n
    # the scan: level k lands at x + 8 y = SCAN8[k]
    c = T8.unscan8(list(range(1, 65)))
    assert c[0][:3] == [1, 2, 6] and c[1][0] == 3 and c[2][0] == 4 and c[7][7] == 64 and c[7][6] == 63 and c[6][7] == 62
    # rows first: the other order gives other samples on most drawn blocks
    g = np.random.default_rng(1)
    differ = 0
    for _ in range(8):
        d = g.integers(-300, 301, size=(8, 8)).tolist()
        t = [list(x) for x in zip(*d)]
        differ += T8.transform8x8(d, RC.Range()) != [list(x) for x in zip(*T8.transform8x8(t, RC.Range()))]
    assert differ >= 4


def test_the_range_watcher_fires():
    b = inter_stim.Builder(2, 1, qp=51)
    pic = b.finish()
    lv = np.zeros(64, np.int64)
    lv[:4] = 32767
    rec = pic.mb_records()
    rec["intra_modes"][0], rec["coef_mask"][0], rec["cbp"][0], rec["coef_index"][0] = N.MB_T8X8, 0xF, 1, 0
    pic.coefs = lv.astype(np.int16)
    pic.desc.n_coef_blocks = 4
    pic.seal()
    out, rng = T8.luma8x8_of(pic, 0, refuse=False)
    assert not rng.ok and "d" in rng.bad
    with pytest.raises(T8.OutOfRange):
        T8.luma8x8_of(pic, 0)
    rec["mb_type"][0] = N.MB_I4x4
    with pytest.raises(AssertionError):
        T8.luma8x8_of(pic, 0)


def test_without_a_flag_it_is_spec_recon():
    stims = inter_stim.b_set()[:2] + inter_stim.shape_set()[:1] + inter_stim.residual_set()[:2] + inter_stim.weighted_set()[:1]
    for st in stims:
        planes = []
        for cls in (spec_recon.SpecRecon, T8.SpecRecon):
            spec = cls(st.pic.mb_w, st.pic.mb_h, 3)
            for slot, f in st.frames.items():
                spec.store.write(slot, f)
            planes.append([p.copy() for p in spec.reconstruct(st.pic)])
        for a, b in zip(*planes):
            assert np.array_equal(a, b), st.name


@pytest.fixture(scope="module")
def sets():
    return {which: getattr(TS, which)() for which in TS.SETS}


@pytest.mark.parametrize("which", TS.SETS)
def test_the_sets_reach_what_they_are_there_for(sets, which):
    TS.assert_covered(which, sets[which])


def test_the_skipped_edges_would_have_been_filtered(sets):
    """the tell: lines of luma edges 1 and 3 of flagged macroblocks that a filter which ignores the flag changes, in both directions"""
    tells = {}
    for st in sets["directed_set"]:
        spec = T8.SpecRecon(st.pic.mb_w, st.pic.mb_h, 3)
        for slot, f in st.frames.items():
            spec.store.write(slot, f)
        spec.reconstruct(st.pic)
        for k, v in spec.tells.items():
            tells[k] = tells.get(k, 0) + v
    assert tells.get("v", 0) >= 50 and tells.get("h", 0) >= 50, tells


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
    st = next(s for s in sets["directed_set"] if s.name.startswith("mixed P"))
    pic, rec = st.pic, st.pic.mb_records()
    fl = np.flatnonzero((rec["intra_modes"] & N.MB_T8X8) != 0)
    coded = next(int(m) for m in fl if rec["coef_mask"][m] & 0xffff)
    intra = int(np.flatnonzero(rec["mb_type"] <= N.MB_I16x16)[0])
    a, b, c = _pack_roads(lib, pic)
    assert a > 0 and b > 0 and c == -1
    good = HipReconstructor.pack_compact(pic, lib)
    hdr = N.CompactHdr.from_buffer_copy(good[:128].tobytes())
    assert lib.p264hip_compact_check(C.byref(pic.desc), good.ctypes.data, good.size) == 0

    def refused(m, field, value, desc_t8=1):
        keep, keep_t8 = rec[field][m], pic.desc.transform_8x8
        rec[field][m], pic.desc.transform_8x8 = value, desc_t8
        bad = good.copy()
        bad[hdr.off_rec + 16 * m:hdr.off_rec + 16 * m + 16] = np.frombuffer(rec[m:m + 1].tobytes(), np.uint8)
        try:
            a, b, c = _pack_roads(lib, pic)
            assert a == -1 and b == -1 and c == m, (field, value, a, b, c)
            assert lib.p264hip_compact_check(C.byref(pic.desc), bad.ctypes.data, bad.size) == -1, (field, value)
        finally:
            rec[field][m], pic.desc.transform_8x8 = keep, keep_t8
    mask = int(rec["coef_mask"][coded])
    k = next(k for k in range(4) if mask >> (4 * k) & 1)
    refused(coded, "coef_mask", mask & ~(1 << (4 * k + 2)))                   # a nibble of 0xB
    refused(coded, "coef_mask", mask & ~(7 << (4 * k)))                      # ... of 0x8
    refused(intra, "intra_modes", int(rec["intra_modes"][intra]) | N.MB_T8X8)  # the flag on an intra record
    refused(int(fl[0]), "qp", int(rec["qp"][fl[0]]), desc_t8=0)              # a flagged record, the descriptor says 0
    a, b, c = _pack_roads(lib, pic)
    assert a > 0 and b > 0 and c == -1


def test_pack_and_compact_round_trips(lib, sets):
    for st in sets["directed_set"][:6] + sets["random_set"]:
        p = st.pic
        plain = HipReconstructor.pack(p, lib)
        view = N.Picture()
        assert lib.p264hip_unpack_input(C.byref(p.desc), plain.ctypes.data, plain.size, C.byref(view)) == 0
        assert view.transform_8x8 == 1
        n, nb = p.n_mb, p.desc.n_coef_blocks
        for name, count, typ in (("mb", n * 16, C.c_uint8), ("coefs", nb * 16, C.c_int16)):
            a = np.ctypeslib.as_array(C.cast(getattr(p.desc, name), C.POINTER(typ)), (count,))
            b = np.ctypeslib.as_array(C.cast(getattr(view, name), C.POINTER(typ)), (count,))
            assert np.array_equal(a, b), (st.name, name)
        comp = HipReconstructor.pack_compact(p, lib)
        back = HipReconstructor.expand_compact(p, comp, lib)
        lay = N.InputLayout()
        lib.p264hip_input_layout(C.byref(p.desc), C.byref(lay))
        for off, size in ((0, n * 16), (lay.off_mv, n * 64), (lay.off_ref, n * 4), (lay.off_i4, n * 16), (lay.off_coef, nb * 32)):
            assert np.array_equal(back[off:off + size], plain[off:off + size]), (st.name, off)


def test_the_kernel_is_in_the_code_object_without_spills_or_scratch(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    assert "k_t8x8" in res, sorted(res)
    r = res["k_t8x8"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r


def test_abi_mirror_of_the_new_fields(lib):
    assert N.LaunchInfo.t8x8_wgs.offset == N.LaunchInfo.deblock_odd_single.offset + 4 and C.sizeof(N.LaunchInfo) == 64
    assert N.Picture.transform_8x8.offset == N.Picture.wp.offset + 384
