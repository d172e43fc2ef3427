"""Directed and random pictures for the 8x8 transform of inter macroblocks (TEST INFRASTRUCTURE), built at the CPU->GPU seam
like tests/inter_stim.py's: everything from seeds, nothing is data.

A picture is first built WITHOUT the luma of the macroblocks that will carry N.MB_T8X8 (inter_stim.Builder or
seam_fuzz.make_picture, brought into range by residual_checker.make_conformant, which reads every record of it), then `insert`
gives those macroblocks the flag, the nibble mask and their 8x8 blocks - four entries each between the chroma DC entry and the
chroma AC entries (include/p264hip.h).  A drawn macroblock whose 8x8 blocks leave the range of 8.5.13 is redrawn with halved
levels (`Stim.redrawn` counts them; the CPU test holds the sets to 10 %).

`directed_set()`: 4 x 3 pictures - a single level at each of the 64 scan positions; every qP % 6 and qP / 6 on both sides of 36;
each quadrant coded alone, all four, none; saturation at 0 and at 255; luma with chroma DC + AC; P 16x16 / 16x8 / 8x16 / 8x8, B
with one list and with two; explicit weights; flagged next to unflagged and intra at all four borders; gradients on which the
skipped edges would have been filtered.  `random_set()`: drawn pictures, 4 x 3, 5 x 1 and 1 x 4, P / B / weighted, several slices."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker as IC
from tests import inter_stim as S
from tests import residual_checker as RC
from tests import seam_fuzz
from tests import t8x8_checker as T8

MB_W, MB_H = S.MB_W, S.MB_H
QPS = ((0, 1, 2, 3, 4, 5, 36, 37, 38, 39, 40, 41), (17, 30, 35, 51, 42, 43, 44, 45, 46, 47, 12, 23))      # every qP % 6 below and from 36; the ends
Stim = collections.namedtuple("Stim", "name pic frames drawn redrawn")     # drawn / redrawn: flagged macroblocks with levels / of them halved


def halve(lv):
    lv = np.asarray(lv, np.int64)
    half = np.where(lv < 0, -((-lv) >> 1), lv >> 1)
    nz = np.flatnonzero(lv)
    if len(nz) and not half.any():
        half[nz[-1]] = 1 if lv[nz[-1]] > 0 else -1             # (a coded block keeps a level)
    return half


def insert(pic, blocks):
    """blocks: {macroblock: {quadrant k: 64 levels in scan order}} ({}: flag set, no block coded).  The macroblocks - inter, without
    luma entries so far - get N.MB_T8X8, their nibbles, cbp bits and entries; the coefficient stream is rebuilt.  Levels that leave the
    range are halved, the macroblock's blocks together.  Returns (macroblocks with levels, of them redrawn)."""
    rec = pic.mb_records()
    old = np.asarray(pic.coefs).reshape(-1, 16)
    out, drawn, redrawn = [], 0, 0
    for m in range(pic.n_mb):
        r = rec[m]
        mask, at = int(r["coef_mask"]), int(r["coef_index"])
        n_old = bin(mask & 0x3ffffff).count("1") if mask else 0
        mine = [old[at + i] for i in range(n_old)]
        new_at = len(out)
        if m in blocks:
            assert int(r["mb_type"]) > N.MB_IPCM and not mask & 0x100ffff, "macroblock %d: inter without luma entries expected" % m
            lv = {k: np.asarray(v, np.int64) for k, v in blocks[m].items()}
            assert all(v.any() and len(v) == 64 for v in lv.values())
            drawn += bool(lv)
            qp, hit = int(r["qp"]), False
            for _ in range(24):
                rng_ = RC.Range()
                for v in lv.values():
                    T8.block8x8(v, qp, rng_)
                if rng_.ok:
                    break
                lv, hit = {k: halve(v) for k, v in lv.items()}, True
            assert rng_.ok
            redrawn += hit
            has_dc = 1 if mask & N.COEF_CHROMA_DC else 0
            luma = [v[16 * j:16 * j + 16].astype(np.int16) for k in sorted(lv) for v in [lv[k]] for j in range(4)]
            mine = mine[:has_dc] + luma + mine[has_dc:]
            r["coef_mask"] = mask | sum(0xF << (4 * k) for k in lv)
            r["cbp"] = (int(r["cbp"]) & 0x30) | sum(1 << k for k in lv)
            r["intra_modes"] = N.MB_T8X8
        r["coef_index"] = new_at
        out += mine
    pic.desc.n_coef_blocks = len(out)
    pic.coefs = np.concatenate(out + [np.zeros(16, np.int16)]).astype(np.int16)
    pic.desc.transform_8x8 = 1
    pic.seal()
    return drawn, redrawn


def draw_block(rng, qp, count=None, top=None):
    """64 levels, `count` non-zero ones (None: drawn, sparse more often than dense) of magnitudes up to `top`.  Both are held to what
    stays in range at qp: a level c scales to about c * v * 2^(qP / 6 - 2) (v <= 58), the two stages multiply a value by up to
    (12 / 8)^2, so count * top <= 1000 / 2^(qP / 6) keeps the sum of everything below 2^15 with room for the stage's intermediates"""
    lv = np.zeros(64, np.int64)
    budget = 1000.0 / 2.0 ** (qp / 6.0)
    count = int(rng.choice([1, 2, 3, 5, 8, 16, 40])) if count is None else count
    count = max(1, min(count, int(budget)))
    top = max(1, min(300 if top is None else top, int(budget / count)))
    pos = rng.choice(64, size=count, replace=False)
    lv[pos] = rng.integers(1, top + 1, size=count) * rng.choice([-1, 1], size=count)
    return lv


def _done(name, b_or_pic, frames, blocks):
    pic = b_or_pic.finish() if isinstance(b_or_pic, S.Builder) else b_or_pic
    if pic.desc.n_coef_blocks:
        RC.make_conformant(pic)
    drawn, redrawn = insert(pic, blocks)
    return Stim(name, pic, frames, drawn, redrawn)


def _chroma(rng, b, m):
    dc = np.zeros(16, np.int64)
    dc[:8] = rng.integers(-6, 7, size=8)
    dc[0] |= 1
    b.levels[m][N.COEF_CHROMA_DC] = dc
    for i in rng.choice(8, size=2, replace=False):
        b.levels[m][1 << (16 + int(i))] = S._some_levels(rng, 15)


def directed_set(seed=8513):
    rng = np.random.default_rng(seed)
    out, n = [], MB_W * MB_H
    # a single level at each scan position, 48 blocks per picture
    for half in range(2):
        b = S.Builder(MB_W, MB_H, qp=int(rng.integers(20, 30)))
        blocks = {}
        for m in range(n):
            b.mv[m] = rng.integers(-12, 13, size=2)
            blocks[m] = {}
            for k in range(4):
                pos = (half * 48 + m * 4 + k) % 64
                lv = np.zeros(64, np.int64)
                lv[pos] = int(rng.integers(8, 25)) * int(rng.choice([-1, 1]))
                blocks[m][k] = lv
        out.append(_done("single levels %d" % half, b, S.frames_for(rng, MB_W, MB_H), blocks))
    # every qP % 6, qP / 6 on both sides of 36; dense and sparse blocks
    for rep in range(2):
        b = S.Builder(MB_W, MB_H)
        blocks = {}
        for m in range(n):
            qp = QPS[rep][m]
            b.pic.rec["qp"][m] = qp
            b.mv[m] = rng.integers(-12, 13, size=2)
            blocks[m] = {k: draw_block(rng, qp, count=(40 if (m + k) & 1 else 3)) for k in range(4) if k != m % 4}
        out.append(_done("qp sweep %d" % rep, b, S.frames_for(rng, MB_W, MB_H), blocks))
    # each quadrant alone, all four, none; with and without chroma DC + AC behind the four-entry groups
    b = S.Builder(MB_W, MB_H, qp=27)
    blocks = {}
    for m in range(n):
        quads = [(0,), (1,), (2,), (3,), (0, 1, 2, 3), (), (0, 3), (1, 2), (0, 1, 2), (3,), (), (0, 1, 2, 3)][m]
        b.mv[m] = rng.integers(-12, 13, size=2)
        if m % 2 == 0 or m == 11:
            _chroma(rng, b, m)
        blocks[m] = {k: draw_block(rng, 27) for k in quads}
    out.append(_done("quadrants", b, S.frames_for(rng, MB_W, MB_H), blocks))
    # saturation: black and white references, a large DC of the sign that leaves 0 .. 255 (and of the other sign)
    for val in (0, 255):
        b = S.Builder(MB_W, MB_H, qp=30)
        blocks = {}
        for m in range(n):
            lv = draw_block(rng, 30, count=4)
            lv[0] = (1 if (val == 255) == (m % 3 != 0) else -1) * int(rng.integers(30, 70))
            blocks[m] = {k: lv.copy() for k in range(4)}
        frames = {s: [np.full((MB_H * 16, MB_W * 16), val, np.uint8), np.full((MB_H * 8, MB_W * 8), val, np.uint8), np.full((MB_H * 8, MB_W * 8), 255 - val, np.uint8)] for s in (1, 2)}
        out.append(_done("saturation at %d" % val, b, frames, blocks))
    # partition shapes of P macroblocks
    b = S.Builder(MB_W, MB_H, qp=24)
    blocks = {}
    for m in range(n):
        shape = ("16x16", "16x8", "8x16", "8x8")[m % 4]
        cells = np.zeros((4, 4, 2), np.int64)
        vec = lambda: rng.integers(-40, 41, size=2)
        if shape == "16x16":
            cells[:] = vec()
        elif shape == "16x8":
            cells[:2], cells[2:] = vec(), vec()
        elif shape == "8x16":
            cells[:, :2], cells[:, 2:] = vec(), vec()
        else:
            b.pic.rec["mb_type"][m] = N.MB_P_8x8
            for q in range(4):
                cells[(q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2] = vec()
        b.mv[m] = cells.reshape(16, 2)
        b.pic.ref_idx[m * 4:m * 4 + 4] = rng.integers(0, 2, size=4) if shape != "16x16" else 1
        if m % 3 == 0:
            _chroma(rng, b, m)
        blocks[m] = {k: draw_block(rng, 24) for k in range(4) if rng.random() < 0.8}
    st = _done("P shapes", b, S.frames_for(rng, MB_W, MB_H), blocks)
    st.pic.shapes = {m: ("16x16", "16x8", "8x16", "8x8")[m % 4] for m in range(n)}
    out.append(st)
    # B pictures road by road (inter_stim.b_set's first picture), default and implicit weights
    for weighted in (0, 1):
        b = S.Builder(MB_W, MB_H, b_picture=True, qp=25)
        b.pic.desc.weighted_bipred = weighted
        mv1 = b.pic.mv_l1.reshape(n, 16, 2)
        r0, r1 = b.pic.ref_idx.reshape(-1, 4), b.pic.ref_idx_l1.reshape(-1, 4)
        blocks = {}
        for m in range(n):
            road = IC.B_ROADS[m % 6]
            vec = lambda: rng.integers(-50, 51, size=2)
            r0[m], r1[m] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            if road == "list0 only":
                r1[m] = -1
                b.mv[m] = vec()
            elif road == "list1 only":
                r0[m] = -1
                for q in range(4):
                    mv1[m, list(IC._quad_blocks(q))] = vec()
            elif road == "generic":
                b.mv[m] = rng.integers(-50, 51, size=(16, 2))
                mv1[m] = rng.integers(-50, 51, size=(16, 2))
            elif road == "second pass whole":
                b.mv[m], mv1[m] = vec(), vec()
            else:
                for q in range(4):
                    b.mv[m, list(IC._quad_blocks(q))], mv1[m, list(IC._quad_blocks(q))] = vec(), vec()
                if road == "second pass with carried quadrants":
                    r1[m, 1], r0[m, 2] = -1, -1
                    mv1[m, list(IC._quad_blocks(1))], b.mv[m, list(IC._quad_blocks(2))] = 0, 0
            if m % 2:
                _chroma(rng, b, m)
            blocks[m] = {k: draw_block(rng, 25) for k in range(4) if rng.random() < 0.8}
        for e0 in range(2):
            for e1 in range(2):
                b.pic.desc.bipred_weight[e0 * N.MAX_REFS + e1] = S.B_WEIGHTS[e0 * 2 + e1]
        out.append(_done("B %s road by road" % ("implicit" if weighted else "default"), b, S.frames_for(rng, MB_W, MB_H), blocks))
    # explicit weights (P and B); flagged beside unflagged and intra at every border (drawn pictures, every second inter macroblock)
    for i, (bp, wp) in enumerate(((False, "legal"), (True, "legal"), (False, None), (True, None))):
        out.append(drawn_picture(rng, "mixed %s%s %d" % ("B" if bp else "P", " weighted" if wp else "", i), MB_W, MB_H, share=0.5, b_picture=bp, explicit_wp=wp,
                                 intra_share=0.25, slices=1, slice_idcs=[0]))
    # ... and with an intra / an unflagged macroblock on each side of a flagged one, whatever the draw
    out.append(drawn_picture(rng, "around intra", MB_W, MB_H, share=1.0, intra_share=0.0, force={5: "i16", 6: "i4"}, slices=1, slice_idcs=[0]))
    out.append(drawn_picture(rng, "around unflagged", MB_W, MB_H, share=1.0, unflagged=(5, 6), intra_share=0.0, slices=1, slice_idcs=[0]))
    # gradients: smooth references, vectors at rest, coded blocks at a QP whose thresholds let the filter work on edges 1 and 3
    for i in range(2):
        b = S.Builder(MB_W, MB_H, qp=38 + 4 * i)
        blocks = {}
        for m in range(n):
            if m % 4 != 3:
                blocks[m] = {k: draw_block(rng, 38 + 4 * i, count=2, top=2) for k in range(4)}
        out.append(_done("gradient %d" % i, b, S.frames_for(rng, MB_W, MB_H, kind="smooth"), blocks))
    return out


def drawn_picture(rng, name, mb_w, mb_h, share=0.6, unflagged=(), **kw):
    """a seam_fuzz picture; `share` of its inter macroblocks (none of `unflagged`) lose their 4x4 luma blocks and get 8x8 ones"""
    kw.setdefault("n_ref", 2)
    kw.setdefault("n_ref_l1", 2)
    kw.setdefault("slots", 3)
    kw.setdefault("dst_slot", 0)
    pic = seam_fuzz.make_picture(rng, mb_w, mb_h, level_style="small", qp_mode="random", mv_range=40, **kw)
    rec = pic.rec
    chosen = [m for m in range(pic.n_mb) if rec["mb_type"][m] > N.MB_IPCM and m not in unflagged and rng.random() < share]
    # take the chosen macroblocks' 4x4 luma entries out of the stream
    old = np.asarray(pic.coefs).reshape(-1, 16)
    out = []
    for m in range(pic.n_mb):
        mask, at = int(rec["coef_mask"][m]), int(rec["coef_index"][m])
        ent = [old[at + i] for i in range(bin(mask & 0x3ffffff).count("1"))] if mask else []
        if m in chosen:
            has_dc = 1 if mask & N.COEF_CHROMA_DC else 0
            n_l = bin(mask & 0xffff).count("1")
            ent = ent[:has_dc] + ent[has_dc + n_l:]
            rec["coef_mask"][m] = mask & ~0xffff
            rec["cbp"][m] = int(rec["cbp"][m]) & 0x30
        rec["coef_index"][m] = len(out)
        out += ent
    pic.desc.n_coef_blocks = len(out)
    pic.coefs = np.concatenate(out + [np.zeros(16, np.int16)]).astype(np.int16)
    pic.seal()
    blocks = {}
    for m in chosen:
        skip = rec["mb_type"][m] == N.MB_P_SKIP
        cbp = 0 if skip else int(rng.integers(0, 16)) if rng.random() < 0.85 else 0
        blocks[m] = {k: draw_block(rng, int(rec["qp"][m])) for k in range(4) if cbp >> k & 1}
    return _done(name, pic, S.frames_for(rng, mb_w, mb_h, kind="smooth" if rng.random() < 0.5 else "noise"), blocks)


def random_set(seed=8514):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(6):
        out.append(drawn_picture(rng, "random %d" % i, MB_W, MB_H, b_picture=bool(i & 1), explicit_wp="legal" if i == 4 else None, intra_share=0.12, slices=1 + i % 3))
    out.append(drawn_picture(rng, "random row 5x1", 5, 1, slices=2))
    out.append(drawn_picture(rng, "random column 1x4", 1, 4, b_picture=True, slices=2))
    return out


SETS = ("directed_set", "random_set")


def assert_covered(which, stims):
    """AssertionError unless the pictures reach what the set is there for (the CPU test on the drawn sets, the GPU file on what it
    submitted)"""
    rec_of = lambda st: st.pic.mb_records()
    fl = lambda st: (rec_of(st)["intra_modes"] & N.MB_T8X8) != 0
    drawn, redrawn = sum(st.drawn for st in stims), sum(st.redrawn for st in stims)
    assert drawn and redrawn * 10 <= drawn, "%s: %d of %d flagged macroblocks redrawn with halved levels" % (which, redrawn, drawn)
    for st in stims:
        assert st.pic.desc.transform_8x8 and fl(st).any(), st.name
        for m in np.flatnonzero(fl(st)):
            assert T8.luma8x8_of(st.pic, int(m), refuse=False)[1].ok, "%s macroblock %d out of range" % (st.name, m)
    if which == "random_set":
        assert {(st.pic.mb_w, st.pic.mb_h) for st in stims} == {(MB_W, MB_H), (5, 1), (1, 4)}
        assert {int(st.pic.desc.slice_type) for st in stims} == {N.SLICE_P, N.SLICE_B} and any(st.pic.desc.explicit_wp for st in stims)
        return
    singles, qps, nibbles, with_chroma, types = set(), set(), set(), set(), set()
    beside = collections.Counter()
    for st in stims:
        rec, f = rec_of(st), fl(st)
        w, h = st.pic.mb_w, st.pic.mb_h
        for m in np.flatnonzero(f):
            r = rec[m]
            mask = int(r["coef_mask"])
            nibbles.add(mask & 0xffff)
            for k in range(4):
                if mask >> (4 * k) & 1:
                    lv = T8.levels8_of(st.pic, r, k)
                    nz = [i for i, v in enumerate(lv) if v]
                    if len(nz) == 1:
                        singles.add(nz[0])
                    qps.add((int(r["qp"]) % 6, int(r["qp"]) // 6 >= 6))
            if mask & 0xffff:
                with_chroma.add((bool(mask & N.COEF_CHROMA_DC), bool(mask & 0xff0000)))
            types.add((int(r["mb_type"]), int(st.pic.desc.slice_type), bool(st.pic.desc.explicit_wp)))
            x, y = m % w, m // w
            for side, ok, nb in (("left", x > 0, m - 1), ("right", x + 1 < w, m + 1), ("top", y > 0, m - w), ("bottom", y + 1 < h, m + w)):
                if not ok:
                    beside[("border", side)] += 1
                elif not f[nb]:
                    beside[("intra" if rec["mb_type"][nb] <= N.MB_IPCM else "unflagged", side)] += 1
    assert singles == set(range(64)), sorted(set(range(64)) - singles)
    assert qps == {(m, hi) for m in range(6) for hi in (False, True)}, sorted(qps)
    assert nibbles >= {0x000f, 0x00f0, 0x0f00, 0xf000, 0xffff, 0}, sorted(hex(x) for x in nibbles)
    assert (True, True) in with_chroma and (False, False) in with_chroma
    assert {t[0] for t in types} >= {N.MB_P_L0, N.MB_P_8x8, N.MB_B} and any(t[2] for t in types)
    for kind in ("border", "intra", "unflagged"):
        for side in ("left", "right", "top", "bottom"):
            assert beside[(kind, side)], (kind, side)
    assert any(st.name.startswith("saturation") for st in stims) and any("shapes" in st.name for st in stims)
