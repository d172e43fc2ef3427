"""tests/inter_checker.py checks itself (CPU): hand-computed samples a reader can hold against H.264 8.4.2.2 without running
anything else; the reference's recorded answers (tests/golden/kat_hotpath.npz: all 1 400 motion-compensation cases, every one of
their 131 200 luma and 2 x 32 800 chroma samples, none excluded; kat_bipred.npz against the two combines); the census - item
kinds, windows, roads - on hand-made macroblocks; and the coverage of the directed pictures of tests/inter_stim.py."""
import os

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import inter_checker as IC
from tests import inter_stim as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_luma_positions_against_hand_computed_samples():
    """a plane that is 10 left of x = 4 and 90 from there on (every row alike): b between the two is (10 - 50 + 200 + 1800 - 450 + 90 +
    16) >> 5 = 50, the quarter positions average it with G = 10 / H = 90; vertically nothing changes"""
    p = np.full((12, 12), 10, np.uint8)
    p[:, 4:] = 90
    at = lambda fx, fy: int(IC.luma_block(p, 3, 5, fx, fy, 1)[0, 0])      # G = p[5, 3] = 10, H = p[5, 4] = 90
    assert at(0, 0) == 10 and at(2, 0) == 50 and at(1, 0) == (10 + 50 + 1) >> 1 and at(3, 0) == (90 + 50 + 1) >> 1
    assert at(0, 2) == 10 and at(0, 1) == 10 and at(0, 3) == 10              # h = G = M
    assert at(2, 2) == 50 and at(2, 1) == 50 and at(2, 3) == 50              # j = b = s
    assert at(1, 1) == 30 and at(1, 3) == 30 and at(1, 2) == 30              # e, p: (b + h + 1) >> 1, (h + s + 1) >> 1; i: (h + j + 1) >> 1
    assert at(3, 1) == 70 and at(3, 3) == 70 and at(3, 2) == 70              # g, r: m = 90 with b / s = 50; k: (j + m + 1) >> 1
    # transposed: the same numbers with the roles of x and y exchanged (G, M instead of G, H)
    t = np.ascontiguousarray(p.T)
    at = lambda fx, fy: int(IC.luma_block(t, 5, 3, fx, fy, 1)[0, 0])
    assert at(0, 2) == 50 and at(0, 1) == 30 and at(0, 3) == 70 and at(2, 0) == 10
    assert at(1, 1) == 30 and at(3, 1) == 30 and at(1, 3) == 70 and at(3, 3) == 70
    # j from the UNCLIPPED intermediates: two bright columns in six dark ones give b1 = 2 * 20 * 255 = 10200 (b = Clip1(319) = 255) in
    # the rows above y = 6 and 0 below: j1 = 10200 * (1 - 5 + 20), j = (163200 + 512) >> 10 = 159; from clipped b's it would be 128
    e = np.zeros((12, 12), np.uint8)
    e[:6, 3:5] = 255
    assert int(IC.luma_block(e, 3, 5, 2, 0, 1)[0, 0]) == 255
    assert int(IC.luma_block(e, 3, 5, 2, 2, 1)[0, 0]) == (10200 * 16 + 512) >> 10 == 159


def test_reference_samples_are_clamped_per_coordinate():
    p = np.arange(64, dtype=np.uint8).reshape(8, 8)
    assert IC.window(p, -3, -2, 5, 4).tolist() == [[0, 0, 0, 0, 1]] * 3 + [[8, 8, 8, 8, 9]]
    assert IC.window(p, 6, 6, 4, 3).tolist() == [[54, 55, 55, 55], [62, 63, 63, 63], [62, 63, 63, 63]]
    assert IC.window(p, 40, -40, 2, 2).tolist() == [[7, 7], [7, 7]]          # wholly outside: the corner sample
    assert int(IC.luma_block(p, -30, 3, 2, 0, 1)[0, 0]) == 24                # six equal samples: (32 * 24 + 16) >> 5


def test_chroma_against_hand_computed_samples():
    p = np.array([[10, 50], [90, 250]], np.uint8)
    at = lambda fx, fy: int(IC.chroma_block(p, 0, 0, fx, fy, 1)[0, 0])
    assert at(0, 0) == 10 and at(4, 0) == 30 and at(0, 4) == 50 and at(4, 4) == 100
    assert at(1, 0) == (7 * 8 * 10 + 8 * 50 + 32) >> 6 and at(0, 1) == (7 * 8 * 10 + 8 * 90 + 32) >> 6     # x weighs B, y weighs C
    assert at(7, 3) == (1 * 5 * 10 + 7 * 5 * 50 + 1 * 3 * 90 + 7 * 3 * 250 + 32) >> 6


def test_the_references_recorded_motion_compensation():
    kat = np.load(os.path.join(GOLDEN, "kat_hotpath.npz"))
    Y, U, V = kat["mc_y"], kat["mc_u"], kat["mc_v"]
    oy = ou = n = 0
    phases, stats = set(), {"j": 0, "j_outside": 0}
    for (mbx, mby, x, y, bw, bh, mvx, mvy) in kat["mc_cases"].tolist():
        ly, lc = 16 * bw * bh, 4 * bw * bh
        X, Yp = mbx * 16 + 4 * x, mby * 16 + 4 * y
        side = 4 * max(bw, bh)
        a = IC.luma_block(Y, X + (mvx >> 2), Yp + (mvy >> 2), mvx & 3, mvy & 3, side, stats)[:4 * bh, :4 * bw]
        assert a.reshape(-1).tolist() == kat["mc_oy"][oy:oy + ly].tolist(), "luma mv (%d, %d) at (%d, %d) %dx%d" % (mvx, mvy, X, Yp, bw, bh)
        for plane, key in ((U, "mc_ou"), (V, "mc_ov")):
            c = IC.chroma_block(plane, X // 2 + (mvx >> 3), Yp // 2 + (mvy >> 3), mvx & 7, mvy & 7, side // 2)[:2 * bh, :2 * bw]
            assert c.reshape(-1).tolist() == kat[key][ou:ou + lc].tolist(), "chroma mv (%d, %d) at (%d, %d)" % (mvx, mvy, X, Yp)
        oy += ly
        ou += lc
        n += 1
        phases.add((mvx & 3, mvy & 3))
    assert (n, oy, ou) == (1400, 131200, 32800) and len(phases) == 16
    assert stats["j"] > 10000 and stats["j_outside"] == 0                    # no centre sample of these cases leaves -80 .. 335


def test_the_references_recorded_combines():
    kat = np.load(os.path.join(GOLDEN, "kat_bipred.npz"))
    pic = type("P", (), {})()
    pic.desc = N.Picture()
    seen = set()
    for a, b, want, (which, w, h, weighted, w1) in zip(kat["a"], kat["b"], kat["out"], kat["par"].tolist()):
        pic.desc.weighted_bipred = weighted
        pic.desc.bipred_weight[0] = w1
        got = IC.combine(pic, a[:h, :w].astype(np.int64), b[:h, :w].astype(np.int64), 0, 0, 0)
        assert np.array_equal(got, want[:h, :w]), "size %dx%d weighted %d w1 %d" % (w, h, weighted, w1)
        seen.add((weighted, w1 < 0, w1 > 64))
    assert {(1, True, False), (1, False, True), (0, False, False)} <= seen


# ---- classification and census on hand-made macroblocks -----------------------------------------------------------------------
def one_mb(b_picture=False):
    b = S.Builder(3, 3, b_picture=b_picture)
    return b, b.pic


def kinds(pic, m):
    items, road = IC.classify(pic, m)
    return {k: v[0] for k, v in items.items()}, road


def test_item_kinds_of_p_macroblocks():
    b, pic = one_mb()
    b.mv[4] = (5, -3)
    assert set(kinds(pic, 4)[0].values()) == {"mb"} and kinds(pic, 4)[1] == "p"
    b.mv[4, 15] = (5, -2)                                    # one block of quadrant 3 differs
    k, _ = kinds(pic, 4)
    assert [k[(0, bb)] for bb in (0, 5, 2, 7, 8, 13)] == ["quad"] * 6 and [k[(0, bb)] for bb in (10, 11, 14, 15)] == ["lane"] * 4
    b.mv[4] = (5, -3)
    pic.ref_idx[4 * 4 + 2] = 1                               # one vector, two references: four quadrant items
    assert set(kinds(pic, 4)[0].values()) == {"quad"}
    pic.ref_idx[4 * 4 + 2] = 7                               # ... an index past the list is entry 0: one item again
    assert set(kinds(pic, 4)[0].values()) == {"mb"}


def test_windows_and_sides():
    b, pic = one_mb()
    # macroblock 0 of a 48 x 48 picture, vector (8, 8) quarter samples: window 21 x 21 at (0, 0), chroma 9 x 9 at (1, 1)
    assert IC.item_window(pic, 0, "mb", tuple(range(16)), (8, 8), False) == (0, 0, 21)
    assert IC.item_window(pic, 0, "mb", tuple(range(16)), (8, 8), True) == (1, 1, 9)
    assert IC.item_window(pic, 8, "quad", (10, 11, 14, 15), (-4, 0), False) == (32 + 8 - 1 - 2, 32 + 8 - 2, 13)
    assert IC._side(0, 21, 48) == ("flush", "in") and IC._side(-1, 21, 48) == ("past", "in") and IC._side(27, 21, 48) == ("in", "flush")
    assert IC._side(28, 21, 48) == ("in", "past") and IC._side(-21, 21, 48) == ("out", "in") and IC._side(48, 21, 48) == ("in", "out")
    c = IC.Census()
    b.mv[0] = (8, 8)
    IC.survey(pic, c)
    assert c.cells[("y", 0, 0, "mb", ("flush", "in", "flush", "in"), "l0", False)] == 16
    assert c.items[("mb", "copy", True, True, False, False)] >= 1


def test_roads_of_b_macroblocks():
    b, pic = one_mb(True)
    mv1 = pic.mv_l1.reshape(-1, 16, 2)
    r0, r1 = pic.ref_idx.reshape(-1, 4), pic.ref_idx_l1.reshape(-1, 4)
    assert kinds(pic, 0)[1] == "list0 only"
    r0[1], r1[1] = -1, 0
    assert kinds(pic, 1)[1] == "list1 only" and set(kinds(pic, 1)[0]) == {(1, bb) for bb in range(16)}
    r1[2] = 0
    mv1[2] = (4, 4)
    k, road = kinds(pic, 2)
    assert road == "second pass whole" and set(k.values()) == {"mb"} and len(k) == 32
    mv1[2, 15] = (4, 5)
    assert kinds(pic, 2)[1] == "generic" and set(kinds(pic, 2)[0].values()) == {"lane"}
    r1[3] = 0
    mv1[3, [10, 11, 14, 15]] = (4, 5)
    k, road = kinds(pic, 3)
    assert road == "second pass quadrants" and k[(0, 0)] == "mb" and k[(1, 0)] == "quad"
    r1[4] = [0, -1, 0, 0]
    k, road = kinds(pic, 4)
    assert road == "second pass with carried quadrants" and (1, 2) not in k and k[(1, 0)] == "quad" and k[(0, 2)] == "quad"


# ---- the directed pictures: every cell is reached -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", [w for w in S.SETS if w != "residual_set"])
def test_directed_sets_reach_every_cell(which):
    S.assert_covered(which, getattr(S, which)())
