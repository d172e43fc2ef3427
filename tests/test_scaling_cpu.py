"""Scaling matrices without a GPU: tests/scaling_checker.py against the checkers it extends (all-16 lists give residual_checker /
t8x8_checker value for value), the default lists, the syntax and fall-back rules of table 7-2, what tests/scaling_stim.py reaches,
and the seam - the descriptor's new fields as C and ctypes see them, the table in the slot layout and in the compact link format,
byte for byte, with flat pictures laid out as they always were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from tests import i8x8_checker as I8
from tests import i8x8_stim as IS
from tests import inter_stim as S
from tests import residual_checker as RC
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import t8x8_checker as T8
from tests import t8x8_stim as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def test_flat_weights_give_the_flat_formulas():
    rng = np.random.default_rng(1)
    w4, w8 = SC.weight4([16] * 16), SC.weight8([16] * 64)
    for qp in range(52):
        c = [[int(v) for v in row] for row in rng.integers(-300, 301, size=(4, 4))]
        a, b = RC.Range(), RC.Range()
        assert SC.scale4x4(c, qp, w4, a) == RC.scale4x4(c, qp, b)
        assert SC.scale4x4(c, qp, w4, a, dc=77) == RC.scale4x4(c, qp, b, dc=77)
        assert SC.luma_dc(c, qp, w4, a) == RC.luma_dc(c, qp, b)
        assert SC.chroma_dc([c[0][0], c[0][1], c[1][0], c[1][1]], qp, w4, a) == RC.chroma_dc([c[0][0], c[0][1], c[1][0], c[1][1]], qp, b)
        c8 = [[int(v) for v in row] for row in rng.integers(-200, 201, size=(8, 8))]
        assert SC.scale8x8(c8, qp, w8, a) == T8.scale8x8(c8, qp, b)
        assert a.n == b.n and a.bad == b.bad


def test_a_weight_scales_its_own_position():
    """one level at scan position k of a list that is 16 but for position k: the scaled block is the flat one times w / 16 at that
    position (qP 28 and 40: shifts left, nothing rounds), for the 4x4 and the 8x8 scan"""
    for k in range(16):
        lst = [16] * 16
        lst[k] = 48
        lv = [0] * 16
        lv[k] = 5
        d = SC.scale4x4(RC.unscan(lv), 28, SC.weight4(lst), RC.Range())
        f = RC.scale4x4(RC.unscan(lv), 28, RC.Range())
        assert d == [[3 * x for x in r] for r in f] and sum(bool(x) for r in d for x in r) == 1
    for k in range(64):
        lst = [16] * 64
        lst[k] = 32
        other = [32] * 64
        other[k] = 16
        lv = [0] * 64
        lv[k] = -3
        f = T8.scale8x8(T8.unscan8(lv), 40, RC.Range())
        assert SC.scale8x8(T8.unscan8(lv), 40, SC.weight8(lst), RC.Range()) == [[2 * x for x in r] for r in f]
        assert SC.scale8x8(T8.unscan8(lv), 40, SC.weight8(other), RC.Range()) == f


def test_the_ends_of_the_byte():
    """weight 0 zeroes its coefficient whatever the level; 255 scales a level to 255 / 16 of its flat value where nothing rounds (qP 28,
    40), and below qP 24 / 36 a weight of 1 leaves the rounding term alone: (c * v + 2^(3 - s)) >> (4 - s); the census files each"""
    assert [SC.weight_class(w) for w in (0, 1, 3, 4, 16, 64, 65, 255)] == ["0", "1..3", "1..3", "4..64", "4..64", "4..64", "65..255", "65..255"]
    for k in range(16):
        lv = [0] * 16
        lv[k] = -7
        for w, mul in ((0, 0), (255, 255)):
            lst = [16] * 16
            lst[k] = w
            seen = SC.Census()
            d = SC.scale4x4(RC.unscan(lv), 28, SC.weight4(lst), RC.Range(), census=seen, n=3)
            f = RC.scale4x4(RC.unscan(lv), 28, RC.Range())
            assert [[16 * x for x in r] for r in d] == [[mul * x for x in r] for r in f]
            assert seen.classes == {(3, SC.weight_class(w)): 1}
    i, j = RC.ZIGZAG[5]
    lst = [16] * 16
    lst[5] = 1
    for qp in range(24):
        lv = [0] * 16
        lv[5] = 3
        d = SC.scale4x4(RC.unscan(lv), qp, SC.weight4(lst), RC.Range())
        assert d[i][j] == (3 * SC.norm4(qp % 6, i, j) + (1 << (3 - qp // 6))) >> (4 - qp // 6) and sum(bool(x) for r in d for x in r) <= 1
    lv = [0] * 64
    lv[9] = 4
    for w in (0, 255):
        lst = [16] * 64
        lst[9] = w
        f = T8.scale8x8(T8.unscan8(lv), 40, RC.Range())
        assert [[16 * x for x in r] for r in SC.scale8x8(T8.unscan8(lv), 40, SC.weight8(lst), RC.Range())] == [[w * x for x in r] for r in f]
    # chroma DC and the Intra16x16 DC line take position 0 of their list
    c4 = [5, -3, 2, 1]
    for w in (0, 1, 255):
        lst = [w] + [16] * 15
        seen = SC.Census()
        got = SC.chroma_dc(c4, 20, SC.weight4(lst), RC.Range(), seen, SC.INTER_CR)
        f = [5 - 3 + 2 + 1, 5 + 3 + 2 - 1, 5 - 3 - 2 - 1, 5 + 3 - 2 + 1]
        assert got == [((x * w * SC.norm4(20 % 6, 0, 0)) << 3) >> 5 for x in f]
        assert seen.dc_classes == {((2, "inter"), SC.weight_class(w)): 1}
        seen = SC.Census()
        dc = SC.luma_dc([[2, 0, 0, 0]] + [[0] * 4] * 3, 30, SC.weight4(lst), RC.Range(), seen)
        assert dc == [[(2 * w * SC.norm4(0, 0, 0) + 1) >> 1] * 4] * 4 and seen.dc_classes == {("luma", SC.weight_class(w)): 1}


def test_flat_pictures_equal_the_checkers_they_extend():
    """scaling_lists = 0, and scaling_lists = 1 with all-16 lists: every macroblock's residual is residual_checker's (4x4, chroma) and
    t8x8_checker's / i8x8_checker's (8x8 blocks)"""
    stims = [S.residual_set()[5], TS.directed_set()[4], IS.inter_set()[0]]
    for st in stims:
        for flag in (0, 1):
            SC.set_lists(st.pic, SS.flat_lists(), flag)
            rec = st.pic.mb_records()
            for m in range(st.pic.n_mb):
                if int(rec["mb_type"][m]) == N.MB_IPCM or not int(rec["coef_mask"][m]):
                    continue
                got = SC.residual_of(st.pic, m)[0]
                if SC.is_8x8(rec[m]):
                    want8 = (I8 if int(rec["mb_type"][m]) <= N.MB_IPCM else T8).luma8x8_of(st.pic, m)[0]
                    assert {k: v for k, v in SC.luma8x8_of(st.pic, m)[0].items()} == want8, (st.name, m)
                    assert {k: v for k, v in got.items() if k[0]} == T8.chroma_residual_of(st.pic, m), (st.name, m)
                else:
                    assert got == RC.residual_of(st.pic, m)[0], (st.name, m)


def test_all_16_lists_decode_as_flat_pictures():
    for a, b in SS.flat_twins(3):
        assert a.changed == 0 and int(a.pic.desc.scaling_lists) == 1 and int(b.pic.desc.scaling_lists) == 0
        assert np.array_equal(a.pic.coefs, b.pic.coefs)
        got = [p.copy() for p in _spec(a)]
        want = [p.copy() for p in _spec(b, I8.SpecRecon)]
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), a.name


def _spec(st, cls=SC.SpecRecon):
    spec = cls(st.pic.mb_w, st.pic.mb_h, 3)
    for slot, f in st.frames.items():
        spec.store.write(slot, f)
    return spec.reconstruct(st.pic)


def test_lists_change_the_picture_and_the_census_sees_them():
    st = SS.scaled(S.residual_set()[2], SS.jvt())
    spec = SC.SpecRecon(st.pic.mb_w, st.pic.mb_h, 3)
    for slot, f in st.frames.items():
        spec.store.write(slot, f)
    got = [p.copy() for p in spec.reconstruct(st.pic)]
    st.pic.desc.scaling_lists = 0
    assert not SC.census(st.pic)[1]                       # (JVT weights at these levels: still in range when flat)
    flat = [p.copy() for p in _spec(st)]
    assert any(not np.array_equal(x, y) for x, y in zip(got, flat))
    assert spec.scaled == 1 and sum(spec.scaling.lists.values()) > 0


# ---- tables 7-2 .. 7-4 ---------------------------------------------------------------------------------------------------------
def test_default_lists():
    assert [sum(x) for x in (SC.DEFAULT_4X4_INTRA, SC.DEFAULT_4X4_INTER, SC.DEFAULT_8X8_INTRA, SC.DEFAULT_8X8_INTER)] == [416, 369, 1680, 1507]
    assert [len(x) for x in SC.DEFAULTS] == SC.SIZES
    for lst in (SC.DEFAULT_8X8_INTRA, SC.DEFAULT_8X8_INTER):
        w = SC.weight8(lst)
        assert all(w[i][j] == w[j][i] for i in range(8) for j in range(8))
        assert w[0][0] == min(lst) and w[7][7] == max(lst)
    for lst in (SC.DEFAULT_4X4_INTRA, SC.DEFAULT_4X4_INTER):
        w = SC.weight4(lst)
        assert all(w[i][j] == w[j][i] for i in range(4) for j in range(4))


def test_the_syntax_of_a_list():
    assert SC.parse_list([8] + [0] * 15, 16) == ([16] * 16, False, 16)
    assert SC.parse_list([-8], 16) == ([8] * 16, True, 1)                      # first nextScale 0: useDefaultScalingMatrixFlag
    lst, dflt, used = SC.parse_list([2, 3, -13], 16)                           # 10, 13, then nextScale 0: the rest repeats 13
    assert (lst, dflt, used) == ([10, 13] + [13] * 14, False, 3)
    assert SC.parse_list([-4, 252], 16)[0][:3] == [4, 4, 4]                      # (4 + 252 + 256) % 256 = 0: ends after one value
    assert SC.parse_list([120, 120, 8], 16)[0][:4] == [128, 248, 248, 248]   # (248 + 8 + 256) % 256 = 0
    for seed in range(6):
        for size in (16, 64):
            lst = [int(v) for v in np.random.default_rng(seed).integers(1, 256, size=size)]
            if seed % 2:
                lst[size // 2:] = [lst[size // 2]] * (size - size // 2)
            d = SC.deltas_of(lst)
            assert SC.parse_list(d, size) == (lst, False, len(d)) and all(-128 <= x <= 127 for x in d)
            assert len(d) == (size if not seed % 2 else size // 2 + 2)


FOLLOW = {0: (1, 2), 1: (2,), 3: (4, 5), 4: (5,)}         # the lists that take list n while they are absent themselves


def test_fall_back_rules_a_and_b():
    r = [SS.random_lists(40)[n] for n in range(8)]
    # rule A, nothing present: the defaults
    assert SC.resolve([None] * 8) == [list(x) for x in SC.DEFAULTS]
    # rule A for every list number: present alone
    for n in range(8):
        coded = [None] * 8
        coded[n] = r[n]
        want = [list(x) for x in SC.DEFAULTS]
        for k in (n,) + FOLLOW.get(n, ()):
            want[k] = r[n]
        assert SC.resolve(coded) == want, n
    # rule B for every list number: absent 0 / 3 / 6 / 7 take the SPS's, the others the list before them
    seq = SC.resolve([r[0], None, r[2], "default", r[4], None, None, r[7]])
    assert seq == [r[0], r[0], r[2], SC.DEFAULT_4X4_INTER, r[4], r[4], SC.DEFAULT_8X8_INTRA, r[7]]
    p = SS.random_lists(41)
    for n in range(8):
        coded = [None] * 8
        coded[n] = p[n]
        got = SC.resolve(coded, seq)
        want = [seq[0], seq[0], seq[0], seq[3], seq[3], seq[3], seq[6], seq[7]]
        want[n] = p[n]
        for k in FOLLOW.get(n, ()):
            want[k] = p[n]
        assert got == want, n
    # a PPS without transform_8x8_mode_flag codes six lists: 6 and 7 fall back
    assert SC.resolve([p[0]] + [None] * 5, seq)[6:] == [seq[6], seq[7]] and SC.resolve([p[0]] + [None] * 5)[6:] == [SC.DEFAULT_8X8_INTRA, SC.DEFAULT_8X8_INTER]
    assert SC.resolve(["default"] * 8, seq) == [list(x) for x in SC.DEFAULTS]
    # the picture's lists
    assert SC.picture_lists() == SS.flat_lists() and SC.picture_lists(sps=[None] * 8) == SC.resolve([None] * 8)
    assert SC.picture_lists(sps=[r[0]] + [None] * 7, pps=[None, p[1]] + [None] * 6)[:3] == [r[0], p[1], p[1]]
    assert SC.picture_lists(pps=[None, p[1]] + [None] * 6)[:3] == [SC.DEFAULT_4X4_INTRA, p[1], p[1]]


# ---- the stimuli ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SS.SETS)
def test_the_sets_reach_what_they_are_there_for(which):
    SS.assert_covered(which, getattr(SS, which)())


# ---- the seam ------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "p264hip.h"
int main(void) {
  printf("pic %zu %zu %zu %zu %zu\n", sizeof(p264hip_picture_t), offsetof(p264hip_picture_t, transform_8x8), offsetof(p264hip_picture_t, scaling_lists),
         offsetof(p264hip_picture_t, scaling4x4), offsetof(p264hip_picture_t, scaling8x8));
  printf("layout %zu %zu %zu\n", sizeof(p264hip_input_layout_t), offsetof(p264hip_input_layout_t, off_wp), offsetof(p264hip_input_layout_t, off_scaling));
  printf("hdr %zu %zu %zu\n", sizeof(p264hip_compact_hdr_t), offsetof(p264hip_compact_hdr_t, off_wp), offsetof(p264hip_compact_hdr_t, off_scaling));
  printf("launch %zu %zu %zu %zu\n", sizeof(p264hip_launch_info_t), offsetof(p264hip_launch_info_t, t8x8_wgs), offsetof(p264hip_launch_info_t, scaled_pictures),
         offsetof(p264hip_launch_info_t, intra_i8));
  printf("bytes %d\n", P264HIP_SCALING_BYTES);
  return 0; }
'''
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I" + INC, c, "-o", exe], check=True)
        out = dict((l.split()[0], [int(x) for x in l.split()[1:]]) for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    P = N.Picture
    assert out["pic"] == [C.sizeof(P), P.transform_8x8.offset, P.scaling_lists.offset, P.scaling4x4.offset, P.scaling8x8.offset]
    assert P.scaling8x8.offset == P.scaling4x4.offset + 96
    assert out["layout"] == [C.sizeof(N.InputLayout), N.InputLayout.off_wp.offset, N.InputLayout.off_scaling.offset]
    assert out["hdr"] == [128, N.CompactHdr.off_wp.offset, N.CompactHdr.off_scaling.offset] and C.sizeof(N.CompactHdr) == 128
    assert out["launch"] == [64, N.LaunchInfo.t8x8_wgs.offset, N.LaunchInfo.scaled_pictures.offset, N.LaunchInfo.intra_i8.offset] and C.sizeof(N.LaunchInfo) == 64
    assert out["bytes"] == [N.SCALING_BYTES] == [224]


def _layout(lib, pic):
    lay = N.InputLayout()
    assert lib.p264hip_input_layout(C.byref(pic.desc), C.byref(lay)) == 0
    return lay


def _cases():
    return [SS.scaled(S.residual_set()[1], SS.random_lists(70)), SS.scaled(S.b_set()[1], SS.ramp_lists()), SS.scaled(S.weighted_set()[0], SS.jvt()),
            SS.scaled(TS.directed_set()[4], SS.random_lists(71)), SS.scaled(IS.inter_set()[0], SS.marked_lists(72))]


def test_the_table_travels_in_the_slot_layout_and_flat_pictures_lie_as_before(lib):
    for st in _cases():
        pic = st.pic
        table = SC.table_bytes(SC.lists_of(pic))
        assert len(table) == N.SCALING_BYTES
        lay = _layout(lib, pic)
        blk = HipReconstructor.pack(pic, lib)
        assert lay.off_scaling and lay.off_scaling % 256 == 0 and lay.bytes == lay.off_scaling + 256 == blk.size
        assert lay.off_scaling >= max(lay.off_coef, lay.off_weights, lay.off_wp) + 1
        assert blk[lay.off_scaling:lay.off_scaling + N.SCALING_BYTES].tobytes() == table
        # unpack: the picture the block holds - its table, whatever the descriptor passed says
        other = N.Picture()
        C.memmove(C.byref(other), C.byref(pic.desc), C.sizeof(N.Picture))
        SC_other = type("P", (), {"desc": other})
        SC.set_lists(SC_other, SS.flat_lists())
        out = N.Picture()
        assert lib.p264hip_unpack_input(C.byref(other), blk.ctypes.data, blk.size, C.byref(out)) == 0
        assert bytes(out.scaling4x4) + bytes(out.scaling8x8) == table and out.scaling_lists == 1
        # the flat copy of the same picture: the layout and the block of before, byte for byte
        pic.desc.scaling_lists = 0
        try:
            flat_lay = _layout(lib, pic)
            flat = HipReconstructor.pack(pic, lib)
        finally:
            pic.desc.scaling_lists = 1
        assert flat_lay.off_scaling == 0 and flat_lay.bytes == lay.off_scaling and flat.size == flat_lay.bytes
        assert all(getattr(flat_lay, n) == getattr(lay, n) for n, _ in N.InputLayout._fields_ if n not in ("bytes", "off_scaling"))
        assert np.array_equal(flat, blk[:flat.size])


def test_the_table_travels_in_the_compact_format_and_flat_blocks_are_as_before(lib):
    for st in _cases():
        pic = st.pic
        table = SC.table_bytes(SC.lists_of(pic))
        blk = HipReconstructor.pack_compact(pic, lib)
        hdr = N.CompactHdr.from_buffer_copy(blk[:128].tobytes())
        assert hdr.off_scaling and hdr.off_scaling % 16 == 0 and hdr.off_scaling + N.SCALING_BYTES == hdr.bytes == blk.size
        assert list(hdr.reserved)[0] == hdr.off_scaling and list(hdr.reserved)[1:] == [0] * 9
        assert blk[hdr.off_scaling:].tobytes() == table
        assert lib.p264hip_compact_header_ok(C.byref(pic.desc), blk.ctypes.data, blk.size) == 1
        assert lib.p264hip_compact_check(C.byref(pic.desc), blk.ctypes.data, blk.size) == 0
        # expansion = the packed block, up to the padding between sections
        exp, packed, lay = HipReconstructor.expand_compact(pic, blk, lib), HipReconstructor.pack(pic, lib), _layout(lib, pic)
        assert exp[lay.off_scaling:lay.off_scaling + N.SCALING_BYTES].tobytes() == table
        n = pic.n_mb
        for off, size in ((lay.off_mb, n * 16), (lay.off_mv, n * 64), (lay.off_ref, n * 4), (lay.off_i4, n * 16), (lay.off_coef, int(pic.desc.n_coef_blocks) * 32)):
            assert np.array_equal(exp[off:off + size], packed[off:off + size])
        # the flat copy: the block of before (the scaled block minus its last section, with off_scaling and bytes of a flat header)
        pic.desc.scaling_lists = 0
        try:
            flat = HipReconstructor.pack_compact(pic, lib)
            fh = N.CompactHdr.from_buffer_copy(flat[:128].tobytes())
            assert fh.off_scaling == 0 and list(fh.reserved) == [0] * 10 and fh.bytes == flat.size == hdr.off_scaling
            assert np.array_equal(flat[128:], blk[128:flat.size])
            assert lib.p264hip_compact_check(C.byref(pic.desc), flat.ctypes.data, flat.size) == 0
            # a flat descriptor refuses the scaled block and the other way round
            assert lib.p264hip_compact_header_ok(C.byref(pic.desc), blk.ctypes.data, blk.size) == 0
        finally:
            pic.desc.scaling_lists = 1
        assert lib.p264hip_compact_header_ok(C.byref(pic.desc), flat.ctypes.data, flat.size) == 0


def test_compact_check_rejects_a_scaling_section_outside_the_block(lib):
    pic = _cases()[0].pic
    blk = HipReconstructor.pack_compact(pic, lib)
    hdr = N.CompactHdr.from_buffer_copy(blk[:128].tobytes())

    def verdicts(off_scaling, size=None):
        bad = blk.copy() if size is None else blk[:size].copy()
        h = N.CompactHdr.from_buffer_copy(bad[:128].tobytes())
        h.off_scaling = off_scaling
        if size is not None:
            h.bytes = size
        bad[:128] = np.frombuffer(bytes(h), np.uint8)
        return lib.p264hip_compact_header_ok(C.byref(pic.desc), bad.ctypes.data, bad.size), lib.p264hip_compact_check(C.byref(pic.desc), bad.ctypes.data, bad.size)
    assert verdicts(hdr.off_scaling) == (1, 0)
    assert verdicts(hdr.off_scaling + 16) == (0, -1)                          # ends behind the block
    assert verdicts(hdr.bytes) == (0, -1)
    assert verdicts(0xfffffff0) == (0, -1)
    assert verdicts(hdr.off_scaling + 4) == (0, -1)                           # not on a 16-byte boundary
    assert verdicts(hdr.off_levels) == (0, -1)                                # inside another section
    assert verdicts(0) == (0, -1)                                             # a scaled picture without its section
    assert verdicts(hdr.off_scaling, blk.size - 16) == (0, -1)                # a block cut short
