"""tests/residual_checker.py checks itself (CPU): hand-computed blocks a reader can hold against H.264 8.5; the reference's
recorded answers on the cases H.264 defines a result for; the layout of include/p264hip.h; make_conformant; and the coverage of
tests/inter_stim.py's residual pictures.

In range = every value the standard bounds (d, e, f, g, h, dcY, dcC, both stages of the DC transforms) lies in -2^15 .. 2^15 - 1 in
exact arithmetic.  Of tests/golden/kat_hotpath.npz that leaves 319 of the 900 `di_*` cases, 111 of the 400 `ldc_*` and 118 of the 400
`cdc_*` - and they stop at QP 32 / 21 / 29: the file draws its levels from +-40 (4x4 blocks) and +-300 (DC blocks) whatever the QP,
and above those QPs every case overflows (the other cases pin the int16 wrap of the reference, SURVEY A-Q8, to the oracle in
tests/test_oracle_kat.py).  tests/golden/kat_residual.npz (make_kat_residual.py: levels that shrink with the quantiser step, 8
cases per QP and family, recorded from the same function tables) carries every QP 0 .. 51 in range in each family."""
import os

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import inter_stim as S
from tests import residual_checker as R
from tests import seam_fuzz

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def mat(a):
    return [[int(a[i * 4 + j]) for j in range(4)] for i in range(4)]


def flat(m):
    return [x for r in m for x in r]


def test_tables():
    assert [R.ZIGZAG.index((i, j)) for i in range(4) for j in range(4)] == [0, 1, 5, 6, 2, 4, 7, 12, 3, 8, 11, 13, 9, 10, 14, 15]   # figure 8-8
    assert [R.level_scale(0, i, j) // 16 for i in range(2) for j in range(2)] == [10, 13, 13, 16] and R.level_scale(5, 3, 3) == 16 * 29
    assert R.level_scale(3, 2, 0) == 16 * 14 and R.level_scale(3, 1, 2) == 16 * 18 and R.level_scale(3, 1, 3) == 16 * 23
    assert [R.chroma_qp(q, 0) for q in (29, 30, 31, 34, 35, 39, 43, 45, 48, 51)] == [29, 29, 30, 32, 33, 35, 37, 38, 39, 39]
    assert R.chroma_qp(5, -12) == 0 and R.chroma_qp(45, 12) == 39 and R.chroma_qp(20, 12) == 31
    assert R.unscan(list(range(1, 17))) == [[1, 2, 6, 7], [3, 5, 8, 13], [4, 9, 12, 14], [10, 11, 15, 16]]
    assert R.unscan(list(range(1, 16)) + [99], ac_only=True) == [[0, 1, 5, 6], [2, 4, 7, 12], [3, 8, 11, 13], [9, 10, 14, 15]]


def test_blocks_against_hand_computed_values():
    g = R.Range()
    # a DC level of 4 at QP 24: d00 = (4 * 10 * 16) << 0, every e, f, g, h = 640, r = (640 + 32) >> 6 = 10
    assert R.block4x4([4] + [0] * 15, 24, g) == [[10] * 4] * 4
    # the two branches of 8.5.12.1: QP 22: (3 * 16 * 16 + 1) >> 1 = 384, QP 24: 3 * 160.  With Flat_4x4_16 every LevelScale4x4 is a
    # multiple of 16 and the lower branch shifts by 4 at most: the division is exact and its rounding term 2^(3 - qP / 6) can never
    # change a result (a decoder without it is not wrong on flat matrices; DESIGN.md lists that mutant as equivalent)
    assert all((c * R.level_scale(q % 6, 1, 1) + (1 << (3 - q // 6))) >> (4 - q // 6) == (c * R.level_scale(q % 6, 1, 1)) >> (4 - q // 6)
               for q in range(24) for c in (-7, -1, 1, 3, 2047))
    assert R.scale4x4(mat([3] + [0] * 15), 22, g)[0][0] == 384 and R.scale4x4(mat([3] + [0] * 15), 24, g)[0][0] == 3 * 160
    assert R.scale4x4(mat([0, 1] + [0] * 14), 47, g)[0][1] == (23 * 16) << 3
    # one level at (0, 1), d = 64: rows: e = (64, 64, 32, -64) .. f0 = (64, 32, -32, -64) in row 0 -> columns copy row 0 into all rows
    assert R.transform4x4([[0, 64, 0, 0]] + [[0] * 4] * 3, g) == [[1, 1, 0, -1]] * 4               # (64, 32, -32, -64) + 32 >> 6
    # ... and at (1, 0): the same down the columns
    assert R.transform4x4([[0] * 4, [64, 0, 0, 0], [0] * 4, [0] * 4], g) == [[1] * 4, [1] * 4, [0] * 4, [-1] * 4]
    # d13 of the second pass: (f1 >> 1) - f3 and f1 + (f3 >> 1) with f1 = 0, f3 = 65 (level at (3, 0)): g2 = -65, g3 = 32 -> h = 32, -65, 65, -32
    assert [r[0] for r in R.transform4x4([[0] * 4, [0] * 4, [0] * 4, [65, 0, 0, 0]], g)] == [(32 + 32) >> 6, (-65 + 32) >> 6, (65 + 32) >> 6, (-32 + 32) >> 6]
    # luma DC, one level 2: f = 2 everywhere; QP 40 (>= 36): (2 * 16 * 16) << 0 = 512; QP 20: (2 * 13 * 16 + 4) >> 3 = 52; QP 1, level 1: rounded
    assert flat(R.luma_dc(mat([2] + [0] * 15), 40, g)) == [512] * 16 and R.luma_dc(mat([2] + [0] * 15), 20, g)[3][3] == 52
    assert R.luma_dc(mat([1] + [0] * 15), 1, g)[0][0] == (11 * 16 + 32) >> 6 == 3                  # truncated: 2
    assert flat(R.luma_dc(mat([0, 2] + [0] * 14), 40, g)) == [512, 512, -512, -512] * 4            # c01: + + - - along a row
    # chroma DC (3, 1, 0, 0): f = (4, 2, 4, 2); QPc 0: (f * 160) >> 5 = 20, 10; odd products are TRUNCATED: f = 1 at QPc 1 -> 176 >> 5 = 5
    assert R.chroma_dc([3, 1, 0, 0], 0, g) == [20, 10, 20, 10] and R.chroma_dc([1, 0, 0, 0], 1, g) == [5] * 4
    assert R.chroma_dc([0, 0, 1, 0], 12, g) == [20, 20, -20, -20]                                   # c10: + on the first row, - on the second
    assert g.ok
    # construction clips
    p = np.array([[250, 3], [100, 100]], np.uint8).repeat(2, 0).repeat(2, 1)
    R.construct(p, 0, 0, [[10, 10, -10, -10]] * 4)
    assert p.tolist() == [[255, 255, 0, 0]] * 2 + [[110, 110, 90, 90]] * 2


def test_range_flags():
    g = R.Range()
    R.scale4x4(mat([300] + [0] * 15), 51, g)                 # 300 * 18 * 16 << 4
    assert g.bad == ["d"]
    g = R.Range()
    R.block4x4([30] * 16, 30, g)                            # every d in range, their sums not
    assert "d" not in g.bad and set(g.bad) & {"e", "f", "g", "h"}
    g = R.Range()
    R.luma_dc(mat([3000] * 16), 0, g)
    assert "luma DC f" in g.bad


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "kat_hotpath.npz")), np.load(os.path.join(GOLDEN, "kat_residual.npz"))


def run_di(k, qps):
    n, seen = 0, set()
    for i, qp in enumerate(qps):
        g = R.Range()
        d = R.scale4x4(mat(k["di_coef"][i]), qp, g)
        r = R.transform4x4(d, g)
        if not g.ok:
            continue
        n += 1
        seen.add(qp)
        assert flat(d) == k["di_deq"][i].tolist(), "scaling, case %d qp %d" % (i, qp)
        p = k["di_dst"][i].reshape(4, 4).copy()
        R.construct(p, 0, 0, r)
        assert p.reshape(-1).tolist() == k["di_rec"][i].tolist(), "transform and construction, case %d qp %d" % (i, qp)
    return n, seen


def run_ldc(k, qps):
    n, seen = 0, set()
    for i, qp in enumerate(qps):
        g = R.Range()
        dc = R.luma_dc(mat(k["ldc_in"][i]), qp, g)
        if g.ok:
            n += 1
            seen.add(qp)
            assert flat(dc) == k["ldc_out"][i].tolist(), "luma DC, case %d qp %d" % (i, qp)
    return n, seen


def run_cdc(k, qps):
    n, seen = 0, set()
    for i, qp in enumerate(qps):
        g = R.Range()
        dc = R.chroma_dc(k["cdc_in"][i], qp, g)
        if g.ok:
            n += 1
            seen.add(qp)
            assert dc == k["cdc_out"][i].tolist(), "chroma DC, case %d qp %d" % (i, qp)
    return n, seen


def test_the_references_recorded_answers_in_range(kat):
    hot, res = kat
    n1, q1 = run_di(hot, hot["di_qp"].tolist())
    n2, q2 = run_ldc(hot, hot["ldc_qp"].tolist())
    n3, q3 = run_cdc(hot, hot["cdc_qp"].tolist())
    assert (n1, n2, n3) == (319, 111, 118)
    assert (max(q1), max(q2), max(q3)) == (32, 21, 29)       # (the module's text: where this file's in-range cases stop)
    qps = res["qp"].tolist()
    m1, r1 = run_di(res, qps)
    m2, r2 = run_ldc(res, qps)
    m3, r3 = run_cdc(res, qps)
    assert min(m1, m2, m3) >= 400 and r1 == r2 == r3 == set(range(52))
    assert (q1 | r1) == (q2 | r2) == (q3 | r3) == set(range(52))


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_blocks_are_found_as_the_header_lays_them_out():
    b = S.Builder(2, 1)
    r = b.pic.rec
    r["mb_type"][0] = N.MB_I16x16
    b.pic.ref_idx[:4] = -1
    b.pic.rec["intra_modes"][0] = 2
    for k, bit in enumerate((1 << 20, N.COEF_CHROMA_DC, 1 << 3, N.COEF_LUMA_DC, 1 << 17, 1 << 0)):
        b.levels[0][bit] = [k + 1] * 16
    b.levels[1][1 << 9] = [9] * 16
    pic = b.finish()
    rec = pic.rec
    assert [R.block_at(rec[0], bit) for bit in (N.COEF_LUMA_DC, N.COEF_CHROMA_DC, 1 << 0, 1 << 3, 1 << 17, 1 << 20)] == [0, 1, 2, 3, 4, 5]
    assert R.levels_of(pic, rec[0], 1 << 17)[0] == 5 and R.levels_of(pic, rec[0], N.COEF_LUMA_DC)[0] == 4
    assert R.block_at(rec[1], 1 << 9) == 6 and int(rec[1]["cbp"]) == 1 << 2 and int(rec[0]["cbp"]) == 15 | 2 << 4
    out, rng, blame = R.residual_of(pic, 1)
    assert list(out) == [(0, 4, 8)]                          # block 9 of the decoding order sits at (1, 2) in units of blocks


def test_which_dc_a_block_takes():
    """Intra16x16: block i takes dcY at its POSITION (dcY[BLK_Y][BLK_X]); chroma: block i of the plane takes dcC[i] (raster); Cb from
    levels 0 .. 3 of the DC block, Cr from 4 .. 7"""
    b = S.Builder(1, 1, qp=40)
    b.pic.rec["mb_type"][0] = N.MB_I16x16
    b.pic.ref_idx[:4] = -1
    b.levels[0][N.COEF_LUMA_DC] = [0, 0, 4] + [0] * 13       # scan position 2 = c10: + in the upper two rows of blocks, - below .. see luma_dc
    b.levels[0][N.COEF_CHROMA_DC] = [0, 2, 0, 0, 0, 0, 2, 0] + [0] * 8
    pic = b.finish()
    out = R.residual_of(pic, 0)[0]
    sign = lambda v: (v > 0) - (v < 0)
    assert [[sign(out[(0, x * 4, y * 4)][0][0]) for x in range(4)] for y in range(4)] == [[1] * 4, [1] * 4, [-1] * 4, [-1] * 4]
    assert [sign(out[(1, x, y)][0][0]) for y in (0, 4) for x in (0, 4)] == [1, -1, 1, -1]         # Cb: c01
    assert [sign(out[(2, x, y)][0][0]) for y in (0, 4) for x in (0, 4)] == [1, 1, -1, -1]         # Cr: c10


# ---- make_conformant ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["wrap", "mixed", "large"])
def test_make_conformant(style):
    rng = np.random.default_rng(77 + len(style))
    pic = seam_fuzz.make_picture(rng, 5, 4, level_style=style, qp_mode="random", n_ref=1, slots=2)
    before = (pic.rec.copy(), pic.coefs.copy())
    n0, flagged = R.census(pic)
    assert flagged, "nothing to do"
    with pytest.raises(R.OutOfRange):
        for m in range(pic.n_mb):
            R.residual_of(pic, m)
    n, changed = R.make_conformant(pic)
    assert n == n0 and 0 < changed <= n
    assert R.census(pic)[1] == {}
    assert np.array_equal(pic.rec, before[0])                # masks, indices, cbp: untouched
    lv = pic.coefs.reshape(-1, 16)
    assert ((lv != 0).any(1) == (before[1].reshape(-1, 16) != 0).any(1)).all(), "a block became all-zero"
    assert (np.abs(lv.astype(int)) <= np.abs(before[1].reshape(-1, 16).astype(int))).all() and (np.sign(lv) * np.sign(before[1].reshape(-1, 16)) >= 0).all()


# ---- the directed residual pictures ---------------------------------------------------------------------------------------------
def test_residual_set_reaches_every_cell_in_range():
    """after make_conformant no block of any directed picture is out of range (the share left out of the comparison with the standard
    is zero) and more than half of the coded blocks are as drawn (inter_stim.assert_covered holds every set to both)"""
    stims = S.residual_set()
    assert len(stims) == 27
    S.assert_covered("residual_set", stims)
