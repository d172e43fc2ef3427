"""High-profile pictures at the edge geometries (TEST INFRASTRUCTURE), drawn at the CPU->GPU seam with tests/i8x8_stim.py's and
tests/scaling_stim.py's means: everything from seeds, nothing is data.

The Intra 8x8, T8X8 and scaled kernel instances ran at 4 x 3, 6 x 5, 8 x 6, 9 x 9 and 11 x 9 macroblocks; the geometry decides code
paths in them (kernel_intra.h: a row is walked in windows of 64 columns, a band of four rows hands its last row to the band below, the
top-right record is taken at min(x + 1, mb_w - 1); kernel_t8x8.h / kernel_scaling.h: two macroblocks per wavefront, the second
guarded by mbi < n_mb).  GEOMETRIES:
    1 x 1     one macroblock: the second half of the only wavefront of k_t8x8 / k_scaled_inter lies past n_mb; one band, three dead rows
    1 x 7     no left or right neighbour anywhere, bands of 4 + 3, min(x + 1, mb_w - 1) == x
    2 x 5     as wide as the 2-macroblock lag between rows; bands of 4 + 1
    9 x 1     a single row: no top neighbour, nothing handed to a band below
    70 x 3    a second 64-column window of six columns, one partial band
    66 x 5    a second window of two columns; the band hand-over (rows 3 -> 4) crosses the window seam

Per geometry five pictures (`picture_set`): a flat P picture with T8X8 inter records and Intra 8x8 macroblocks among them (every fourth
macroblock; in the wide geometries columns 63, 64 and the last of every row as well), a flat dense I picture (i8x8_stim.dense_picture's
pattern: Intra 8x8 with Intra4x4, Intra16x16 and I_PCM between), a B picture with the JVT lists, a P picture with random lists and
explicit weights, a dense I picture with ramp_lists().  At 1 x 1 the kinds are split over more pictures: the one macroblock is a T8X8
inter record in one P picture and Intra 8x8 in another, Intra 8x8 in one I picture and Intra16x16 / I_PCM in others.  Stimuli are drawn
streams' way: every picture of a set carries T8X8_INTRA in transform_8x8, as every picture of a High-profile stream with
transform_8x8_mode_flag does."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import i8x8_stim as IS
from tests import pcm_fuzz
from tests import residual_checker as RC
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import seam_fuzz
from tests import t8x8_stim as TS

# drawn / redrawn: 8x8-flagged macroblocks with levels / of them redrawn with halved levels (i8x8_stim, t8x8_stim); changed: level blocks
# scaling_checker.make_conformant had to shrink for the picture's lists
Stim = collections.namedtuple("Stim", "name pic frames drawn redrawn changed")
GEOMETRIES = ((1, 1), (1, 7), (2, 5), (9, 1), (70, 3), (66, 5))
SEED = 9100
WINDOW = 64                   # columns of a window of intra_kernel's row walk
BAND = 4                      # rows of a band of it


def flagged_of(mb_w, mb_h):
    """the macroblocks of a P / B picture that are forced Intra4x4 and converted: every fourth; rows 3 and 4 of column 0, on both sides
    of the hand-over between bands; and columns 63, 64 and the last of every row of a picture wider than a window"""
    out = {m for m in range(mb_w * mb_h) if m % 4 == 0}
    if mb_h > BAND:
        out |= {(BAND - 1) * mb_w, BAND * mb_w}
    if mb_w > WINDOW:
        out |= {y * mb_w + x for y in range(mb_h) for x in (WINDOW - 1, WINDOW, mb_w - 1)}
    return tuple(sorted(out))


def _flat(st):
    return Stim(st.name, st.pic, st.frames, st.drawn, st.redrawn, 0)


def _scaled(st, lists):
    sc = SS.scaled(st, lists)
    return Stim(sc.name, sc.pic, sc.frames, st.drawn, st.redrawn, sc.changed)


def single_intra(rng, plan, name, kind):
    """an I picture of 1 x 1: the macroblock Intra 8x8 ("i8"), Intra16x16 ("i16") or I_PCM ("ipcm")"""
    pic = seam_fuzz.make_picture(rng, 1, 1, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[0], force={0: "i16" if kind == "i16" else "i4"})
    if kind == "ipcm":
        pcm_fuzz.to_ipcm(rng, pic, 0, samples="noise", chosen=np.ones(1, bool))
    RC.make_conformant(pic)
    drawn, redrawn = IS.convert(pic, rng, {0} if kind == "i8" else set(), plan, first=1)
    return IS.Stim(name, pic, {}, drawn, redrawn)


def single_inter(rng, plan, name, i8, **kw):
    """a P or B picture of 1 x 1: the macroblock Intra 8x8, or an inter record with P264_MB_T8X8 (i8x8_stim.inter_picture for one macroblock)"""
    st = TS.drawn_picture(rng, name, 1, 1, share=1.0, intra_share=0.0, force={0: "i4"} if i8 else {}, slices=1, slice_idcs=[0], **kw)
    if i8:
        st.pic.desc.transform_8x8 = 0                      # (no inter record carries the flag: Intra 8x8 alone)
    drawn, redrawn = IS.convert(st.pic, rng, {0} if i8 else set(), plan, first=1)
    return IS.Stim(name, st.pic, st.frames, st.drawn + drawn, st.redrawn + redrawn)


def with_levels(draw, tries=24):
    """draw() until the picture's 8x8-flagged macroblocks carry levels (a single macroblock may be drawn skipped or without a coded block)"""
    for _ in range(tries):
        st = draw()
        if st.drawn:
            return st
    raise AssertionError("no picture with levels in %d draws" % tries)


def single_set(rng):
    plan = IS.Plan(rng)
    p = lambda name, i8, **kw: with_levels(lambda: single_inter(rng, plan, name, i8, **kw))
    i = lambda name, kind: single_intra(rng, plan, name, kind)
    return [_flat(p("P T8X8 1x1", False)), _flat(p("P Intra 8x8 1x1", True)),
            _flat(with_levels(lambda: i("I Intra 8x8 1x1", "i8"))), _flat(i("I Intra16x16 1x1", "i16")), _flat(i("I I_PCM 1x1", "ipcm")),
            _scaled(p("B T8X8 JVT 1x1", False, b_picture=True), SS.jvt()),
            _scaled(p("P T8X8 weighted random lists 1x1", False, explicit_wp="legal"), SS.random_lists(SEED + 1)),
            _scaled(p("P Intra 8x8 random lists 1x1", True), SS.random_lists(SEED + 2)),
            _scaled(with_levels(lambda: i("I Intra 8x8 ramp 1x1", "i8")), SS.ramp_lists()), _scaled(i("I Intra16x16 ramp 1x1", "i16"), SS.ramp_lists())]


def picture_set(mb_w, mb_h, seed=SEED):
    """the pictures of one geometry, flat ones first"""
    rng = np.random.default_rng([seed, mb_w, mb_h])
    if (mb_w, mb_h) == (1, 1):
        return single_set(rng)
    plan, size, flagged = IS.Plan(rng), "%dx%d" % (mb_w, mb_h), flagged_of(mb_w, mb_h)
    p = lambda name, **kw: IS.inter_picture(rng, plan, "%s %s" % (name, size), flagged, 0.7, mb_w, mb_h, slices=1, slice_idcs=[0], **kw)
    i = lambda name: IS.dense_picture(rng, plan, "%s %s" % (name, size), True, mb_w, mb_h)
    return [_flat(p("P flat")), _flat(i("dense I flat")),
            _scaled(p("B JVT", b_picture=True), SS.jvt()), _scaled(p("P weighted random lists", explicit_wp="legal"), SS.random_lists(seed + mb_w)),
            _scaled(i("dense I ramp"), SS.ramp_lists())]


def is_scaled(st):
    return bool(int(st.pic.desc.scaling_lists))


def runs_k_t8x8(st):
    """the picture alone makes a flat batch launch k_t8x8 (batch_fill in p264hip.hip fills BatchKinds.t8, launch_plan.h turns it into the launch)"""
    return bool(int(st.pic.desc.transform_8x8) & ~N.T8X8_INTRA) and int(st.pic.desc.slice_type) != N.SLICE_I


def assert_covered(geometry, stims):
    """AssertionError unless the pictures (all of one geometry) hold what the geometry is on the list for: the CPU test on the drawn
    sets, the GPU file on what it sent"""
    mb_w, mb_h = geometry
    assert stims and {(st.pic.mb_w, st.pic.mb_h) for st in stims} == {geometry}
    # the suite's caps: 8x8 macroblocks redrawn with halved levels, level blocks shrunk for the lists; nothing out of range
    drawn, redrawn = sum(st.drawn for st in stims), sum(st.redrawn for st in stims)
    assert drawn and redrawn * 10 <= drawn, "%s: %d of %d macroblocks redrawn with halved levels" % (geometry, redrawn, drawn)
    changed, blocks = sum(st.changed for st in stims), sum(int(st.pic.desc.n_coef_blocks) for st in stims)
    assert changed * 5 <= blocks, "%s: %d of %d level blocks shrunk" % (geometry, changed, blocks)
    seen = SS.survey(stims)                                                   # (raises on a level block out of range)
    kinds, i8_at, t8_at, types = set(), set(), set(), set()
    for st in stims:
        d, rec = st.pic.desc, st.pic.mb_records()
        assert int(d.transform_8x8) & N.T8X8_INTRA, st.name
        kinds.add((int(d.slice_type), is_scaled(st), bool(d.explicit_wp)))
        for m in range(st.pic.n_mb):
            t, flags, coded = int(rec["mb_type"][m]), int(rec["intra_modes"][m]), bool(int(rec["coef_mask"][m]) & 0xffff)
            types.add(t if t <= N.MB_IPCM else "inter")
            if t == N.MB_I4x4 and flags & N.MB_I8X8:
                i8_at.add((m % mb_w, m // mb_w, int(d.slice_type), is_scaled(st), coded))
            if t > N.MB_IPCM and flags & N.MB_T8X8:
                assert runs_k_t8x8(st)
                t8_at.add((m % mb_w, m // mb_w, is_scaled(st), coded))
    assert kinds >= {(N.SLICE_P, False, False), (N.SLICE_I, False, False), (N.SLICE_B, True, False), (N.SLICE_P, True, True), (N.SLICE_I, True, False)}, kinds
    n_plain = sum(((m % mb_w) + 3 * (m // mb_w)) % 4 == 0 for m in range(mb_w * mb_h))         # (dense_picture: the macroblocks that stay I4x4 / I16x16 / I_PCM by turns)
    assert types >= {N.MB_I4x4, N.MB_I16x16, "inter"} and (N.MB_IPCM in types or 1 < n_plain < 3), types
    # Intra 8x8 macroblocks with levels in I and in P / B pictures, flat and scaled; T8X8 records with levels, flat and scaled
    for scaled in (False, True):
        assert any(c and s == scaled and t == N.SLICE_I for _, _, t, s, c in i8_at) and any(c and s == scaled and t != N.SLICE_I for _, _, t, s, c in i8_at), (geometry, scaled)
        assert any(c and s == scaled for _, _, s, c in t8_at), (geometry, scaled)
    assert seen.lists[SC.INTRA_Y8] > 0 and seen.lists[SC.INTER_Y8] > 0 and (mb_w <= WINDOW or all(seen.lists[n] > 0 for n in range(8))), dict(seen.lists)
    i8_xy, t8_xy = {(x, y) for x, y, _, _, _ in i8_at}, {(x, y) for x, y, _, _ in t8_at}
    # Intra 8x8 in every row, both kinds in every band; the picture's last macroblock (where n_mb is odd the other half of its wavefront
    # in k_t8x8 / k_scaled_inter lies past n_mb) is one or the other
    assert {y for _, y in i8_xy} == set(range(mb_h)), (geometry, sorted(i8_xy))
    assert {y // BAND for _, y in t8_xy} == {y // BAND for y in range(mb_h)}, (geometry, sorted(t8_xy))
    assert (mb_w - 1, mb_h - 1) in i8_xy | t8_xy
    if mb_w > WINDOW:
        # both sides of the window seam and the last column: in every row of a flat and of a scaled picture, and in an I picture
        for x in (WINDOW - 1, WINDOW, mb_w - 1):
            for scaled in (False, True):
                assert {b for a, b, _, s, _ in i8_at if a == x and s == scaled} == set(range(mb_h)), "%s: column %d, scaled %s" % (geometry, x, scaled)
            assert any(a == x and t == N.SLICE_I for a, _, t, _, _ in i8_at), "%s: no Intra 8x8 macroblock of an I picture in column %d" % (geometry, x)
    if mb_h > BAND:
        # the hand-over between bands: one picture with Intra 8x8 macroblocks above and below it in one column - behind the window seam
        # where there is one
        first = WINDOW if mb_w > WINDOW else 0
        for st in stims:
            rec = st.pic.mb_records()
            f = [(int(rec["mb_type"][m]) == N.MB_I4x4 and bool(int(rec["intra_modes"][m]) & N.MB_I8X8)) for m in range(st.pic.n_mb)]
            if any(f[(BAND - 1) * mb_w + x] and f[BAND * mb_w + x] for x in range(first, mb_w)):
                return
        raise AssertionError("%s: no picture with Intra 8x8 macroblocks on both sides of the band seam in one column from %d" % (geometry, first))
