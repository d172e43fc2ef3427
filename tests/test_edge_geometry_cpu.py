"""tests/edge_geometry_stim.py without a GPU: every geometry's set is drawn, stays inside the suite's caps (8x8 macroblocks redrawn with
halved levels: a tenth; level blocks shrunk for the lists: a fifth), has a clean range census and holds what the geometry is on the
list for - Intra 8x8 macroblocks and T8X8 records in every band, in columns 63, 64 and the last of the wide pictures and on both sides
of the band seam; the sets are seeds and nothing else; the width and height arguments i8x8_stim's pictures got leave its sets what
they were (tests/test_distinct_pool_cpu.py and tests/golden/high_pool.json hold their digests)."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import edge_geometry_stim as E
from tests import i8x8_stim as IS
from tests import scaling_checker as SC
from tests import seam_fuzz


@pytest.fixture(scope="module")
def sets():
    return {g: E.picture_set(*g) for g in E.GEOMETRIES}


def test_the_geometries_are_the_ones_the_kernels_branch_on():
    assert E.GEOMETRIES == ((1, 1), (1, 7), (2, 5), (9, 1), (70, 3), (66, 5))
    for w, h in E.GEOMETRIES:
        wins, bands = -(-w // E.WINDOW), -(-h // E.BAND)
        assert (wins, w - (wins - 1) * E.WINDOW, bands, h - (bands - 1) * E.BAND) == {(1, 1): (1, 1, 1, 1), (1, 7): (1, 1, 2, 3), (2, 5): (1, 2, 2, 1), (9, 1): (1, 9, 1, 1),
                                                                                   (70, 3): (2, 6, 1, 3), (66, 5): (2, 2, 2, 1)}[(w, h)]
    assert E.flagged_of(70, 3) == tuple(sorted({m for m in range(210) if m % 4 == 0} | {y * 70 + x for y in range(3) for x in (63, 64, 69)}))
    assert {3, 4} <= set(E.flagged_of(1, 7)) and {6, 8} <= set(E.flagged_of(2, 5)) and {3 * 66, 4 * 66} <= set(E.flagged_of(66, 5))      # rows 3 and 4 of column 0


@pytest.mark.parametrize("geometry", E.GEOMETRIES, ids=lambda g: "%dx%d" % g)
def test_a_geometry_holds_what_it_is_there_for(sets, geometry):
    stims = sets[geometry]
    assert len(stims) == (10 if geometry == (1, 1) else 5)
    scaled = [E.is_scaled(st) for st in stims]
    assert scaled == sorted(scaled) and scaled.count(True) == (5 if geometry == (1, 1) else 3)           # flat ones first
    E.assert_covered(geometry, stims)
    # the census of every picture by itself: level blocks, none out of range
    for st in stims:
        n, out = SC.census(st.pic)
        assert not out and (n or int(st.pic.mb_records()["mb_type"][0]) == N.MB_IPCM), st.name
    if geometry[0] > E.WINDOW:
        # Intra 8x8 in columns 63, 64 and the last; rows 3 and 4 of 66 x 5
        for st in stims:
            rec = st.pic.mb_records()
            at = {(m % geometry[0], m // geometry[0]) for m in np.flatnonzero((rec["intra_modes"] & N.MB_I8X8) != 0)}
            assert {x for x, _ in at} >= {63, 64, geometry[0] - 1}, st.name
            if geometry[1] > E.BAND:
                assert {y for x, y in at if x >= 63} >= {3, 4}, st.name


def test_the_sets_are_their_seeds(sets):
    for g in ((1, 1), (2, 5)):
        again = E.picture_set(*g)
        assert [seam_fuzz.picture_digest(st.pic) for st in again] == [seam_fuzz.picture_digest(st.pic) for st in sets[g]]
    assert len({seam_fuzz.picture_digest(st.pic) for stims in sets.values() for st in stims}) == sum(len(s) for s in sets.values())


def test_one_macroblock_is_every_kind_once(sets):
    """1 x 1: the one macroblock is a T8X8 inter record, Intra 8x8 in P and in I pictures, Intra16x16 and I_PCM, flat and scaled"""
    kinds = set()
    for st in sets[(1, 1)]:
        r = st.pic.mb_records()[0]
        t, flags = int(r["mb_type"]), int(r["intra_modes"])
        kind = "ipcm" if t == N.MB_IPCM else "i16" if t == N.MB_I16x16 else "i8" if t == N.MB_I4x4 and flags & N.MB_I8X8 else "t8" if t > N.MB_IPCM and flags & N.MB_T8X8 else "other"
        assert kind == "ipcm" or int(r["coef_mask"]), st.name
        kinds.add((kind, int(st.pic.desc.slice_type), E.is_scaled(st)))
    assert kinds == {("t8", N.SLICE_P, False), ("i8", N.SLICE_P, False), ("i8", N.SLICE_I, False), ("i16", N.SLICE_I, False), ("ipcm", N.SLICE_I, False),
                     ("t8", N.SLICE_B, True), ("t8", N.SLICE_P, True), ("i8", N.SLICE_P, True), ("i8", N.SLICE_I, True), ("i16", N.SLICE_I, True)}, kinds


def test_the_default_sizes_draw_the_pictures_of_before():
    """width and height passed as what they default to: the same picture, bit for bit"""
    a, b = np.random.default_rng(5), np.random.default_rng(5)
    x = IS.inter_picture(a, IS.Plan(a), "x", IS.CLUSTER, 0.5, slices=1, slice_idcs=[0])
    y = IS.inter_picture(b, IS.Plan(b), "x", IS.CLUSTER, 0.5, IS.MB_W, IS.MB_H, slices=1, slice_idcs=[0])
    assert seam_fuzz.picture_digest(x.pic) == seam_fuzz.picture_digest(y.pic) and (x.pic.mb_w, x.pic.mb_h) == (6, 5)
    a, b = np.random.default_rng(6), np.random.default_rng(6)
    x, y = IS.dense_picture(a, IS.Plan(a)), IS.dense_picture(b, IS.Plan(b), mb_w=IS.DENSE_W, mb_h=IS.DENSE_H)
    assert seam_fuzz.picture_digest(x.pic) == seam_fuzz.picture_digest(y.pic) and (x.pic.mb_w, x.pic.mb_h) == (9, 9)
