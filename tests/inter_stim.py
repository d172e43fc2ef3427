"""Directed pictures for inter prediction and the residual (TEST INFRASTRUCTURE): small pictures at the CPU->GPU seam, built per
cell of what tests/inter_checker.py's census and this module's residual survey record, instead of hoping that random vectors
land one sample from a border.  Everything is generated from seeds; nothing is data.

* `window_set()`: k_mc decides "window inside the picture / clamped" per work item with a window test (kernel_mc_sort.h, mc_classify;
  windows in tests/inter_checker.py).  On pictures of 4 x 3 macroblocks, for each of the seven phase classes and each item kind -
  whole macroblock, quadrant, and the per-block fetch of quadrants whose vectors differ (the eighth class) - one item each with its
  luma window flush with each border, one sample past each border, in all four corners (flush and past), wholly outside on each
  side, and the same for the chroma window (a chroma window flush left is a luma window past the border: luma clamped, chroma
  inside); every case once without and once with coded blocks (luma and chroma).  Any macroblock can reach any border with the
  right vector, so twelve cases share a picture (quadrant cases four per macroblock, per-block cases sixteen).
* `phase_set()`: all sixteen (xFrac, yFrac) x chroma eighths 0 .. 7 in x and y (the low three bits of both components: 64
  pairs), as macroblock items, quadrant items and per-block fetches, with integer parts of both signs.
* `shape_set()`: every partition shape down to 4x4; a 2 x 18 picture (a second band of sixteen macroblock rows), 11 x 1 and 1 x 9.
* `b_set()`: B pictures that reach the six roads of the stage (inter_checker.B_ROADS), with the default and with implicit
  weights, weights -64, negative, 128 among them, near and far vectors.
* `limit_set()`: vectors at the limits H.264 allows, -8192 .. 8191 quarter samples horizontally, -2048 .. 2047 vertically.
* `weighted_set()`: P and B pictures with explicit weight tables.
* `residual_set()`: every QP 0 .. 51 in Intra16x16, Intra4x4 and inter macroblocks, chroma_qp_offset -12 .. 12 (qPI clipped at 0 and
  at 51, every step of table 8-15), blocks with >= 8 levels, one level at each scan position, DC only, AC only, DC + AC, in
  Intra16x16, Intra4x4, inter luma, Cb and Cr.
Every picture with levels goes through residual_checker.make_conformant; `Stim.kept` = (coded blocks, blocks it changed)."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker as IC
from tests import residual_checker as RC
from tests import seam_fuzz

MB_W, MB_H = 4, 3
Stim = collections.namedtuple("Stim", "name pic frames kept")     # frames: {slot: [y, u, v]} of the reference slots
FRACTIONS = {"copy": [(0, 0)], "h": [(1, 0), (2, 0), (3, 0)], "v": [(0, 1), (0, 2), (0, 3)], "diag": [(1, 1), (3, 1), (1, 3), (3, 3)],
             "c": [(2, 2)], "ch": [(2, 1), (2, 3)], "cv": [(1, 2), (3, 2)]}
PLACES = (["flush " + s for s in ("left", "right", "top", "bottom")] + ["past " + s for s in ("left", "right", "top", "bottom")] +
          [k + " corner " + c for k in ("flush", "past") for c in ("tl", "tr", "bl", "br")] + ["outside " + s for s in ("left", "right", "top", "bottom")])
DECODE_AT = {(seam_fuzz.BLK_X[i], seam_fuzz.BLK_Y[i]): i for i in range(16)}


class Builder:
    """a picture of inter macroblocks with vector 0 to start with; per macroblock the level blocks {coef_mask bit: int[16]}"""

    def __init__(self, mb_w, mb_h, b_picture=False, qp=26, deblock=True, chroma_qp_offset=0):
        self.pic = seam_fuzz.SeamPicture(mb_w, mb_h)
        d = self.pic.desc
        d.slice_type = N.SLICE_B if b_picture else N.SLICE_P
        d.chroma_qp_offset = chroma_qp_offset
        d.deblock = int(deblock)
        d.dst_slot = 0
        d.n_ref = 2
        d.ref_slot[0], d.ref_slot[1] = 1, 2
        if b_picture:
            d.n_ref_l1 = 2
            d.ref_slot_l1[0], d.ref_slot_l1[1] = 2, 1
        n = mb_w * mb_h
        self.levels = [dict() for _ in range(n)]
        rec = self.pic.rec
        for m in range(n):
            x, y = m % mb_w, m // mb_w
            rec["mb_type"][m] = N.MB_B if b_picture else N.MB_P_L0
            rec["qp"][m] = qp
            rec["avail"][m] = ((N.AVAIL_LEFT if x else 0) | (N.AVAIL_TOP if y else 0) | (N.AVAIL_TOPRIGHT if y and x + 1 < mb_w else 0) |
                               (N.AVAIL_TOPLEFT if x and y else 0))
            rec["edges"][m] = (N.EDGE_INNER | (N.EDGE_LEFT if x else 0) | (N.EDGE_TOP if y else 0)) if deblock else 0
        self.mv = self.pic.mv.reshape(n, 16, 2)           # [macroblock][4x4 block, raster][x, y]

    def finish(self):
        pic, rec = self.pic, self.pic.rec
        blocks = []
        for m, lv in enumerate(self.levels):
            mask = 0
            for bit in lv:
                mask |= bit
            cbp_l = 15 if (rec["mb_type"][m] == N.MB_I16x16 and mask & 0xffff) else 0 if rec["mb_type"][m] == N.MB_I16x16 else \
                sum(1 << q for q in range(4) if mask >> (4 * q) & 15)
            cc = 2 if mask & 0xff0000 else 1 if mask & N.COEF_CHROMA_DC else 0
            rec["coef_mask"][m] = mask
            rec["cbp"][m] = cbp_l | cc << 4
            rec["coef_index"][m] = len(blocks)
            order = sorted(lv, key=lambda b: -2 if b == N.COEF_LUMA_DC else -1 if b == N.COEF_CHROMA_DC else b)
            blocks += [np.asarray(lv[b], np.int16) for b in order]
        pic.desc.n_coef_blocks = len(blocks)
        if blocks:
            pic.coefs = np.concatenate(blocks).astype(np.int16)
        return pic.seal()


def frames_for(rng, mb_w, mb_h, slots=(1, 2), kind="noise"):
    return {s: seam_fuzz.random_frame(rng, mb_w, mb_h, kind) for s in slots}


def _stim(name, pic, frames):
    kept = RC.make_conformant(pic) if pic.desc.n_coef_blocks else (0, 0)
    return Stim(name, pic, frames, kept)


stim = _stim                           # (public names: tests/worklist_stim.py draws its macroblocks with them)


def _some_levels(rng, n=16, count=3, top=9):
    lv = np.zeros(16, np.int64)
    pos = rng.choice(n, size=count, replace=False)
    lv[pos] = rng.integers(1, top + 1, size=count) * rng.choice([-1, 1], size=count)
    return lv


some_levels = _some_levels


def _code_item(rng, b, m, raster_blocks):
    """coded luma blocks inside the item (one or two of its 4x4 blocks) and chroma DC + one AC block"""
    pick = [raster_blocks[int(i)] for i in rng.choice(len(raster_blocks), size=min(2, len(raster_blocks)), replace=False)]
    for bb in pick:
        b.levels[m][1 << DECODE_AT[(bb & 3, bb >> 2)]] = _some_levels(rng)
    dc = np.zeros(16, np.int64)
    dc[:8] = rng.integers(-6, 7, size=8)
    dc[0] |= 1
    b.levels[m][N.COEF_CHROMA_DC] = dc
    b.levels[m][1 << int(rng.integers(16, 24))] = _some_levels(rng, 15)


def _target(rng, place, n, size_x, size_y, chroma):
    """top-left of a window of n samples for the place, the other dimension well inside"""
    def inside(size):
        return int(rng.integers(2, size - n - 1))
    wx, wy = inside(size_x), inside(size_y)
    kind, _, where = place.partition(" ")
    far = n + int(rng.integers(0, 7))
    if "corner" in where:
        c = where.split()[1]
        o = 0 if kind == "flush" else 1
        wx = -o if c[1] == "l" else size_x - n + o
        wy = -o if c[0] == "t" else size_y - n + o
        return wx, wy
    o = {"flush": 0, "past": 1, "outside": far}[kind]
    if where == "left":
        wx = -o
    elif where == "right":
        wx = size_x - n + o
    elif where == "top":
        wy = -o
    else:
        wy = size_y - n + o
    return wx, wy


def _vector(wx, wy, x0, y0, frac, chroma, rng):
    """the vector that puts the item at (x0, y0) (luma samples) onto the window (wx, wy) with the luma fractions `frac`"""
    if not chroma:
        return (wx + 2 - x0) * 4 + frac[0], (wy + 2 - y0) * 4 + frac[1]
    return (wx - x0 // 2) * 8 + frac[0] + 4 * int(rng.integers(0, 2)), (wy - y0 // 2) * 8 + frac[1] + 4 * int(rng.integers(0, 2))


vector_onto = _vector


def window_set(seed=8422):
    rng = np.random.default_rng(seed)
    W, H = MB_W * 16, MB_H * 16
    cases = {"mb": [], "quad": [], "lane": []}
    for kind in cases:
        for pc in IC.PHASE_CLASSES:
            k = 0
            for chroma in (False, True):
                for place in PLACES:
                    if chroma and ("corner" in place or place.startswith("outside")):
                        continue
                    for coded in (False, True):
                        cases[kind].append((pc, FRACTIONS[pc][k % len(FRACTIONS[pc])], chroma, place, coded))
                        k += 1
    out, n_mb = [], MB_W * MB_H
    todo = {k: list(v) for k, v in cases.items()}

    def take(kind, coded):
        """the next case of the kind with that `coded` (the residual bits of the keys are per quadrant for luma, per macroblock
        for chroma: the cases that share a macroblock share the flag); a picture's spare places repeat earlier cases"""
        for i, c in enumerate(todo[kind]):
            if c[4] == coded:
                return todo[kind].pop(i)
        same = [c for c in cases[kind] if c[4] == coded]
        return same[int(rng.integers(0, len(same)))]
    for kind in ("mb", "quad", "lane"):
        while todo[kind]:
            b = Builder(MB_W, MB_H, qp=int(rng.integers(18, 34)))
            for m in range(n_mb):
                X0, Y0 = (m % MB_W) * 16, (m // MB_W) * 16
                if kind != "mb":
                    b.pic.rec["mb_type"][m] = N.MB_P_8x8
                b.pic.ref_idx[m * 4:m * 4 + 4] = int(rng.integers(0, 2))
                mb_coded = todo[kind][0][4] if todo[kind] else bool(m & 1)
                for q in range(4 if kind != "mb" else 1):
                    qb = IC._quad_blocks(q) if kind != "mb" else tuple(range(16))
                    units = [(bb,) for bb in qb] if kind == "lane" else [qb]
                    coded_any = False
                    for blocks in units:
                        pc, frac, chroma, place, coded = take(kind, mb_coded)
                        x0, y0 = X0 + (blocks[0] & 3) * 4, Y0 + (blocks[0] >> 2) * 4
                        n = (IC.CHROMA_WINDOW if chroma else IC.LUMA_WINDOW)[kind][0]
                        wx, wy = _target(rng, place, n, W >> chroma, H >> chroma, chroma)
                        v = _vector(wx, wy, x0, y0, frac, chroma, rng)
                        for bb in blocks:
                            b.mv[m, bb] = v
                        coded_any |= coded
                    if kind == "lane" and len({tuple(b.mv[m, bb]) for bb in qb}) == 1:
                        b.mv[m, qb[3]] += (4, 0)                           # (four equal draws: keep the quadrant differing)
                    if coded_any:
                        _code_item(rng, b, m, list(qb))
                if kind == "quad" and len({tuple(x) for x in b.mv[m].tolist()}) == 1:
                    b.mv[m, 15] += (0, 4)
                    b.mv[m, 14], b.mv[m, 11], b.mv[m, 10] = b.mv[m, 15], b.mv[m, 15], b.mv[m, 15]
            out.append(_stim("window %s %d" % (kind, len(out)), b.finish(), frames_for(rng, MB_W, MB_H)))
    return out


def phase_set(seed=8423):
    rng = np.random.default_rng(seed)
    pairs = [(fx, fy) for fy in range(8) for fx in range(8)]
    out = []
    for kind, per in (("mb", 1), ("quad", 4), ("lane", 16)):
        todo = list(pairs)
        while todo:
            b = Builder(MB_W, MB_H, qp=28)
            for m in range(MB_W * MB_H):
                if kind != "mb":
                    b.pic.rec["mb_type"][m] = N.MB_P_8x8
                for q in range(4 if kind != "mb" else 1):
                    qb = IC._quad_blocks(q) if kind != "mb" else tuple(range(16))
                    for blocks in ([(bb,) for bb in qb] if kind == "lane" else [qb]):
                        fx, fy = todo.pop(0) if todo else pairs[int(rng.integers(0, 64))]
                        v = (int(rng.integers(-3, 4)) * 8 + fx, int(rng.integers(-3, 4)) * 8 + fy)
                        for bb in blocks:
                            b.mv[m, bb] = v
                    if kind == "lane" and len({tuple(b.mv[m, bb]) for bb in qb}) == 1:
                        b.mv[m, qb[3]] += (8, 0)
                if kind == "quad" and len({tuple(x) for x in b.mv[m].tolist()}) == 1:
                    for bb in IC._quad_blocks(3):
                        b.mv[m, bb] += (0, 8)
            out.append(_stim("phases %s %d" % (kind, len(out)), b.finish(), frames_for(rng, MB_W, MB_H)))
    return out


SHAPES = ("16x16", "16x8", "8x16", "8x8", "8x4", "4x8", "4x4", "mixed sub")


def shape_set(seed=8424):
    rng = np.random.default_rng(seed)
    b = Builder(MB_W, MB_H, qp=24)
    shapes = {}
    for m in range(MB_W * MB_H):
        shape = SHAPES[m % len(SHAPES)]
        shapes[m] = shape
        cells = np.zeros((4, 4, 2), np.int64)

        def vec():
            return rng.integers(-60, 61, size=2)
        if shape == "16x16":
            cells[:] = vec()
        elif shape == "16x8":
            cells[:2], cells[2:] = vec(), vec()
        elif shape == "8x16":
            cells[:, :2], cells[:, 2:] = vec(), vec()
        else:
            b.pic.rec["mb_type"][m] = N.MB_P_8x8
            for q in range(4):
                qy, qx = (q >> 1) * 2, (q & 1) * 2
                sub = {"8x8": 0, "8x4": 1, "4x8": 2, "4x4": 3}.get(shape, q)
                if sub == 0:
                    cells[qy:qy + 2, qx:qx + 2] = vec()
                elif sub == 1:
                    cells[qy, qx:qx + 2], cells[qy + 1, qx:qx + 2] = vec(), vec()
                elif sub == 2:
                    cells[qy:qy + 2, qx], cells[qy:qy + 2, qx + 1] = vec(), vec()
                else:
                    cells[qy:qy + 2, qx:qx + 2] = rng.integers(-60, 61, size=(2, 2, 2))
        b.mv[m] = cells.reshape(16, 2)
        b.pic.ref_idx[m * 4:m * 4 + 4] = rng.integers(0, 2, size=4) if shape not in ("16x16",) else 0
        if m % 2:
            _code_item(rng, b, m, list(range(16)))
    out = [_stim("partition shapes", b.finish(), frames_for(rng, MB_W, MB_H))]
    out[0].pic.shapes = shapes
    for name, w, h, kw in (("two bands 2x18", 2, 18, dict(slices=2)), ("single row 11x1", 11, 1, dict(slices=3)), ("single column 1x9", 1, 9, dict(slices=4))):
        for i in range(2):
            pic = seam_fuzz.make_picture(rng, w, h, n_ref=2, slots=3, dst_slot=0, level_style="small", qp_mode="random", b_picture=bool(i), n_ref_l1=2, **kw)
            out.append(_stim("%s %s" % (name, "B" if i else "P"), pic, frames_for(rng, w, h)))
    return out


B_WEIGHTS = [-64, 128, -17, 40]              # bipred_weight of the pairs (0, 0), (0, 1), (1, 0), (1, 1)


def b_set(seed=8425):
    """drawn B pictures (seam_fuzz.make_picture: every direction per quadrant, vectors per macroblock / quadrant / block); the
    coverage test holds the set to the six roads under both kinds of weight"""
    rng = np.random.default_rng(seed)
    out = []
    for weighted in (0, 1):
        # one picture built road by road: two macroblocks per road, one of them with coded blocks
        b = Builder(MB_W, MB_H, b_picture=True, qp=25)
        b.pic.desc.weighted_bipred = weighted
        mv1 = b.pic.mv_l1.reshape(MB_W * MB_H, 16, 2)
        r0, r1 = b.pic.ref_idx.reshape(-1, 4), b.pic.ref_idx_l1.reshape(-1, 4)
        for m in range(MB_W * MB_H):
            road = IC.B_ROADS[m % 6]

            def vec():
                return rng.integers(-70, 71, size=2)
            r0[m], r1[m] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            if road == "list0 only":
                r1[m] = -1
                b.mv[m] = vec()
            elif road == "list1 only":
                r0[m] = -1
                for q in range(4):
                    mv1[m, list(IC._quad_blocks(q))] = vec()
            elif road == "generic":
                b.mv[m] = rng.integers(-70, 71, size=(16, 2))
                mv1[m] = rng.integers(-70, 71, size=(16, 2))
            elif road == "second pass whole":
                b.mv[m], mv1[m] = vec(), vec()
            else:
                for q in range(4):
                    b.mv[m, list(IC._quad_blocks(q))], mv1[m, list(IC._quad_blocks(q))] = vec(), vec()
                if road == "second pass with carried quadrants":
                    r1[m, 1], r0[m, 2] = -1, -1
                    mv1[m, list(IC._quad_blocks(1))], b.mv[m, list(IC._quad_blocks(2))] = 0, 0
            if m >= 6:
                _code_item(rng, b, m, list(range(16)))
        for e0 in range(2):
            for e1 in range(2):
                b.pic.desc.bipred_weight[e0 * N.MAX_REFS + e1] = B_WEIGHTS[e0 * 2 + e1]
        out.append(_stim("B %s road by road" % ("implicit" if weighted else "default"), b.finish(), frames_for(rng, MB_W, MB_H)))
        for mv_range, n in ((10, 3), (300, 2)):
            for i in range(n):
                pic = seam_fuzz.make_picture(rng, MB_W, MB_H, n_ref=2, slots=3, dst_slot=0, level_style="small", qp_mode="random", b_picture=True,
                                             n_ref_l1=2, weighted=bool(weighted), mv_range=mv_range, intra_share=0.08, past_list=0.1 if i == 1 else 0.0)
                for e0 in range(2):
                    for e1 in range(2):
                        pic.desc.bipred_weight[e0 * N.MAX_REFS + e1] = B_WEIGHTS[e0 * 2 + e1]
                out.append(_stim("B %s range %d #%d" % ("implicit" if weighted else "default", mv_range, i), pic, frames_for(rng, MB_W, MB_H)))
    return out


LIMITS_X, LIMITS_Y = (-8192, -8191, 8190, 8191), (-2048, -2045, 2046, 2047)


def limit_set(seed=8426):
    rng = np.random.default_rng(seed)
    out = []
    for kind in ("mb", "quad", "lane"):
        b = Builder(MB_W, MB_H, qp=27)
        for m in range(MB_W * MB_H):
            if kind != "mb":
                b.pic.rec["mb_type"][m] = N.MB_P_8x8

            def vec():
                k = int(rng.integers(0, 3))
                vx = LIMITS_X[int(rng.integers(0, 4))] if k != 1 else int(rng.integers(-40, 41))
                vy = LIMITS_Y[int(rng.integers(0, 4))] if k != 0 else int(rng.integers(-40, 41))
                return vx, vy
            if kind == "mb":
                b.mv[m] = [(LIMITS_X[m % 4], int(rng.integers(-40, 41))), (int(rng.integers(-40, 41)), LIMITS_Y[m % 4]), (LIMITS_X[m % 4], LIMITS_Y[(m + 1) % 4])][m // 4]
            else:
                for q in range(4):
                    qb = IC._quad_blocks(q)
                    if kind == "quad":
                        v = vec()
                        for bb in qb:
                            b.mv[m, bb] = v
                    else:
                        for bb in qb:
                            b.mv[m, bb] = vec()
                        if len({tuple(b.mv[m, bb]) for bb in qb}) == 1:
                            b.mv[m, qb[0]] = (17, -9)
                if len({tuple(x) for x in b.mv[m].tolist()}) == 1:
                    b.mv[m, 0] = (5, 6)
            if m % 3 == 0:
                _code_item(rng, b, m, list(range(16)))
        out.append(_stim("vector limits %s" % kind, b.finish(), frames_for(rng, MB_W, MB_H)))
    return out


def weighted_set(seed=8427):
    rng = np.random.default_rng(seed)
    out = []
    for i, (bp, mode, rngv) in enumerate(((False, "legal", 12), (False, "wide", 300), (True, "legal", 12), (True, "legal", 300), (True, "wide", 40))):
        pic = seam_fuzz.make_picture(rng, MB_W, MB_H, n_ref=2, slots=3, dst_slot=0, level_style="small", qp_mode="random", b_picture=bp, n_ref_l1=2,
                                     explicit_wp=mode, mv_range=rngv, intra_share=0.08, dup_refs=(i == 2))
        out.append(_stim("explicit weights %s %s range %d" % ("B" if bp else "P", mode, rngv), pic, frames_for(rng, MB_W, MB_H)))
    return out


# ---- the residual -----------------------------------------------------------------------------------------------------------
PATTERNS = ["dense"] + ["single %d" % k for k in range(16)] + ["dc only", "ac only", "dc+ac"]
KINDS = ("i16", "i4", "inter", "cb", "cr")


def _magnitude(rng, qp):
    return max(1, int(rng.integers(1, 300) / 2.0 ** (max(qp - 12, 0) / 6.0)))


def _pattern_levels(rng, pattern, qp, n):
    """n = 16 (full block) or 15 (AC-only block: scan position k is level k - 1); None where the pattern has no such block"""
    lv = np.zeros(16, np.int64)

    def put(positions):
        for p in positions:
            lv[p] = _magnitude(rng, qp) * int(rng.choice([-1, 1]))
    if pattern == "dense":
        put(rng.choice(n, size=int(rng.integers(8, n + 1)), replace=False))
    elif pattern.startswith("single"):
        k = int(pattern.split()[1])
        if n == 15:
            if k == 0:
                return None
            k -= 1
        put([k])
    elif n == 16:
        put({"dc only": [0], "ac only": rng.choice(np.arange(1, 16), size=3, replace=False), "dc+ac": [0] + list(rng.choice(np.arange(1, 16), size=3, replace=False))}[pattern])
    else:
        if pattern == "dc only":
            return None
        put(rng.choice(15, size=3, replace=False))
    return lv


def residual_set(seed=8428):
    rng = np.random.default_rng(seed)
    out = []
    types = (N.MB_I16x16, N.MB_I4x4, N.MB_P_L0)
    k = 0
    for offset in range(-12, 13):
        b = Builder(MB_W, MB_H, chroma_qp_offset=offset)
        for m in range(MB_W * MB_H):
            qp = k % 52 if k < 156 else (k * 5 + 3) % 52            # with the type's rotation: every (type, QP) in the first 156
            if abs(offset) >= 9 and m % 4 == 0:                     # the ends of the offsets' range: qPI clipped at 0 and at 51
                qp = m // 4 if offset < 0 else 51 - m // 4
                if m == 0 and abs(offset) == 9:                     # ... and qPI exactly 0 / 51, unclipped
                    qp = 9 if offset < 0 else 42
            t = types[(k + k // 52) % 3]
            pat = PATTERNS[(k * 11 + k // 20) % len(PATTERNS)]
            cpat = PATTERNS[(k * 7 + 3 + k // 20) % len(PATTERNS)]
            k += 1
            r = b.pic.rec
            r["mb_type"][m], r["qp"][m] = t, qp
            lv = b.levels[m]
            if t != N.MB_P_L0:
                b.pic.ref_idx[m * 4:m * 4 + 4] = -1
                r["intra_modes"][m] = 2 if t == N.MB_I16x16 else 0                  # Intra16x16 DC, chroma DC: legal everywhere
            else:
                b.mv[m] = rng.integers(-20, 21, size=2)
            if t == N.MB_I16x16:
                # the DC block takes the pattern's DC side, the AC blocks its AC side
                if pat != "ac only":
                    dc = _pattern_levels(rng, pat if pat.startswith("single") or pat == "dense" else "dense" if pat == "dc+ac" else "single %d" % int(rng.integers(0, 16)), qp, 16)
                    lv[N.COEF_LUMA_DC] = dc
                if pat != "dc only":
                    for i in rng.choice(16, size=int(rng.integers(1, 6)), replace=False):
                        a = _pattern_levels(rng, pat, qp, 15)
                        if a is not None:
                            lv[1 << int(i)] = a
            else:
                for i in rng.choice(16, size=int(rng.integers(2, 7)), replace=False):
                    lv[1 << int(i)] = _pattern_levels(rng, pat, qp, 16)
            qpc = RC.chroma_qp(qp, offset)
            if cpat != "ac only":
                dc = np.zeros(16, np.int64)
                for ch in range(2):
                    if cpat.startswith("single"):
                        dc[ch * 4 + int(cpat.split()[1]) % 4] = _magnitude(rng, qpc) * int(rng.choice([-1, 1]))
                    else:
                        dc[ch * 4:ch * 4 + 4] = [_magnitude(rng, qpc) * int(rng.choice([-1, 0, 1])) for _ in range(4)]
                        dc[ch * 4] |= 1
                lv[N.COEF_CHROMA_DC] = dc
            if cpat != "dc only":
                for i in rng.choice(8, size=int(rng.integers(1, 5)), replace=False):
                    a = _pattern_levels(rng, cpat, qpc, 15)
                    if a is not None:
                        lv[1 << (16 + int(i))] = a
        out.append(_stim("residual offset %d" % offset, b.finish(), frames_for(rng, MB_W, MB_H, kind="smooth")))
    # where the DC branches round: LevelScale(m, 0, 0) = 16 v, so dcC = (f v 2^(QPc / 6)) >> 1 is truncated only when QPc < 6 and f v is
    # odd (v = 11, 13: QPc 1, 2), and dcY's rounding term counts only below QP 12.  A dcY / dcC that is off by one shows in the samples
    # only where it crosses (h + 32) >> 6 of 8.5.12.2: blocks without AC levels whose right value is 32 (luma) / 31 (chroma) modulo 64 -
    # one DC level (f = that level for every block) searched for per QP; chroma_qp_offset 0
    for rep in range(2):
        b = Builder(MB_W, MB_H, chroma_qp_offset=0)
        for m in range(MB_W * MB_H):
            r = b.pic.rec
            qp = m if rep == 0 else 1 + m % 2
            r["mb_type"][m], r["qp"][m], r["intra_modes"][m] = N.MB_I16x16, qp, 2
            b.pic.ref_idx[m * 4:m * 4 + 4] = -1
            ls, sh = RC.level_scale(qp % 6, 0, 0), 6 - qp // 6
            good = [f for f in range(-400, 401) if ((f * ls + (1 << (sh - 1))) >> sh) % 64 == 32 and (f * ls) >> sh != (f * ls + (1 << (sh - 1))) >> sh]
            if good:
                dc = np.zeros(16, np.int64)
                dc[0] = good[int(rng.integers(0, len(good)))]
                b.levels[m][N.COEF_LUMA_DC] = dc
            good = [f for f in range(-400, 401) if ((f * ls) >> 5) % 64 == 31 and (f * ls) >> 5 != (f * ls + 16) >> 5] if qp < 6 else []
            if good:
                cdc = np.zeros(16, np.int64)
                cdc[0], cdc[4] = good[int(rng.integers(0, len(good)))], good[int(rng.integers(0, len(good)))]
                b.levels[m][N.COEF_CHROMA_DC] = cdc
        out.append(_stim("residual DC rounding %d" % rep, b.finish(), frames_for(rng, MB_W, MB_H, kind="smooth")))
    return out


def residual_survey(pic, seen):
    """raises the sets of `seen` (new_residual_survey): what the picture's coded blocks exercise, from its arrays alone"""
    rec = pic.mb_records()
    off = int(pic.desc.chroma_qp_offset)
    for m in range(pic.n_mb):
        t, qp, mask = int(rec["mb_type"][m]), int(rec["qp"][m]), int(rec["coef_mask"][m])
        if t == N.MB_IPCM or not mask:
            continue
        kind = "i16" if t == N.MB_I16x16 else "i4" if t == N.MB_I4x4 else "inter"

        def lv(bit):
            return RC.levels_of(pic, rec[m], bit)

        def pattern(levels, first):
            nz = [i + first for i, v in enumerate(levels) if v]
            out = set()
            if len(nz) >= 8:
                out.add("dense")
            if len(nz) == 1:
                out.add("single %d" % nz[0])
            return out
        if mask & 0x0100ffff:
            seen["qp"].add((kind, qp % 6, qp // 6))
        if kind == "i16":
            has_dc = bool(mask & N.COEF_LUMA_DC)
            if has_dc:
                seen["pattern"] |= {("i16", p) for p in pattern(lv(N.COEF_LUMA_DC), 0)}
                seen["luma_dc_branch"].add(qp >= 36)
                if qp < 36:                                         # dcY values that a truncating decoder gets wrong
                    ls, sh = RC.level_scale(qp % 6, 0, 0), 6 - qp // 6
                    f = RC.luma_dc_transform(RC.unscan(lv(N.COEF_LUMA_DC)), RC.Range())
                    for i in range(16):                             # (blocks without AC levels: h = dcY in every sample)
                        fx = f[RC.BLK_Y[i]][RC.BLK_X[i]]
                        seen["tells"]["luma DC rounded"] += not mask >> i & 1 and (((fx * ls + (1 << (sh - 1))) >> sh) + 32) >> 6 != (((fx * ls) >> sh) + 32) >> 6
            for i in range(16):
                ac = bool(mask >> i & 1)
                if ac:
                    seen["pattern"] |= {("i16", p) for p in pattern(lv(1 << i)[:15], 1)}
                if ac or has_dc:
                    seen["pattern"].add(("i16", "dc+ac" if ac and has_dc else "ac only" if ac else "dc only"))
        else:
            for i in range(16):
                if mask >> i & 1:
                    l = lv(1 << i)
                    seen["pattern"] |= {(kind, p) for p in pattern(l, 0)}
                    if any(l):
                        seen["pattern"].add((kind, "dc only" if not any(l[1:]) else "ac only" if not l[0] else "dc+ac"))
        if mask & 0x0000ffff or (kind == "i16" and mask & N.COEF_LUMA_DC):
            seen["scale_branch"].add((kind, qp >= 24))
        if int(rec["cbp"][m]) >> 4:
            qpi = qp + off
            seen["qpi"].add("low" if qpi < 0 else "high" if qpi > 51 else qpi)
            qpc = RC.chroma_qp(qp, off)
            seen["qpc"].add((qpc % 6, qpc // 6))
            has_dc = bool(mask & N.COEF_CHROMA_DC)
            for ch, name in ((0, "cb"), (1, "cr")):
                if has_dc:
                    seen["pattern"] |= {(name, p) for p in pattern(lv(N.COEF_CHROMA_DC)[ch * 4:ch * 4 + 4], 0)}
                    c = lv(N.COEF_CHROMA_DC)[ch * 4:ch * 4 + 4]
                    ls = RC.level_scale(qpc % 6, 0, 0)
                    for i, fx in enumerate((c[0] + c[1] + c[2] + c[3], c[0] - c[1] + c[2] - c[3], c[0] + c[1] - c[2] - c[3], c[0] - c[1] - c[2] + c[3])):
                        t = (fx * ls) << (qpc // 6)                 # dcC values that a rounding decoder gets wrong, in blocks without AC levels
                        seen["tells"]["chroma DC truncated"] += not mask >> (16 + ch * 4 + i) & 1 and ((t >> 5) + 32) >> 6 != (((t + 16) >> 5) + 32) >> 6
                for i in range(4):
                    b = 16 + ch * 4 + i
                    ac = bool(mask >> b & 1)
                    if ac:
                        seen["pattern"] |= {(name, p) for p in pattern(lv(1 << b)[:15], 1)}
                    if ac or has_dc:
                        seen["pattern"].add((name, "dc+ac" if ac and has_dc else "ac only" if ac else "dc only"))
    return seen


def new_residual_survey():
    return dict(qp=set(), pattern=set(), qpi=set(), qpc=set(), luma_dc_branch=set(), scale_branch=set(), tells=collections.Counter())


def residual_cells():
    """what residual_set has to reach: {name of the set in the survey: the cells}"""
    pat = {(k, p) for k in KINDS for p in PATTERNS}
    return dict(qpc={(q % 6, q // 6) for q in range(40)},
                qp={(k, a, b) for k in ("i16", "i4", "inter") for a in range(6) for b in range(9) if b * 6 + a < 52},
                pattern=pat, qpi={"low", "high"} | set(range(52)), luma_dc_branch={False, True},
                scale_branch={(k, f) for k in ("i16", "i4", "inter") for f in (False, True)})


# ---- coverage of the inter sets ---------------------------------------------------------------------------------------------
def window_cells():
    """the census cells window_set has to reach, as predicates' keys: (kind, phase class or 'any' for the per-block fetch, plane,
    place, coded)"""
    cells = set()
    for kind in ("mb", "quad", "lane"):
        for pc in IC.PHASE_CLASSES:
            for plane in "yc":
                for place in PLACES:
                    if plane == "c" and ("corner" in place or place.startswith("outside")):
                        continue
                    for coded in (False, True):
                        cells.add((kind, pc, plane, place, coded))
    return cells


def _place_of(sides):
    """the places (PLACES) a window with these (left, right, top, bottom) sides stands for"""
    names = ("left", "right", "top", "bottom")
    out = set()
    for i, s in enumerate(sides):
        if s == "out":
            out.add("outside " + names[i])
    if out:
        return out
    for i, s in enumerate(sides):
        if s in ("flush", "past") and all(o == "in" for j, o in enumerate(sides) if j != i):
            out.add(s + " " + names[i])
    for c, (a, b) in (("tl", (2, 0)), ("tr", (2, 1)), ("bl", (3, 0)), ("br", (3, 1))):
        for k in ("flush", "past"):
            if sides[a] == k and sides[b] == k:
                out.add("%s corner %s" % (k, c))
    return out


def window_reached(census):
    """the window_cells a census (inter_checker.Census) holds"""
    got = set()
    for (plane, fx, fy, kind, sides, lists, coded), n in census.cells.items():
        pc = IC.phase_class(fx & 3, fy & 3)
        for place in _place_of(sides):
            got.add((kind, pc, plane, place, coded))
    return got


# ---- what every set has to hold (the CPU tests on the drawn sets, the GPU file on what it submitted) ----------------------------
SETS = ("window_set", "phase_set", "shape_set", "b_set", "limit_set", "weighted_set", "residual_set")


def assert_covered(which, stims):
    """AssertionError unless the pictures `stims` of the set `which` reach every cell the set is there for, hold no block outside
    the range H.264 bounds, and kept at least half of their coded blocks as drawn"""
    c = IC.Census()
    for st in stims:
        IC.survey(st.pic, c)
        assert not RC.census(st.pic)[1], "%s: blocks out of range after make_conformant" % st.name
    coded, changed = sum(st.kept[0] for st in stims), sum(st.kept[1] for st in stims)
    assert changed <= coded // 2, "%s: only %d of %d coded blocks kept the levels they were drawn with" % (which, coded - changed, coded)
    every = [(x, y) for x in range(4) for y in range(4)]
    if which == "window_set":
        assert all((st.pic.mb_w, st.pic.mb_h) == (MB_W, MB_H) for st in stims)
        missing = window_cells() - window_reached(c)
        assert not missing, "%d cells not reached, e.g. %s" % (len(missing), sorted(missing)[:8])
        # the keys of k_mc's lists: phase class x inside / clamped x residual or not per item kind; luma clamped with chroma inside
        for kind in ("mb", "quad"):
            for pc in IC.PHASE_CLASSES:
                for inside in (False, True):
                    for coded_ in (False, True):
                        assert any(k[:3] == (kind, pc, inside) and k[4] == coded_ for k in c.items), (kind, pc, inside, coded_)
                        assert any(k[:2] == (kind, pc) and k[3] == inside and k[5] == coded_ for k in c.items), (kind, pc, "chroma", inside, coded_)
                assert any(k[:2] == (kind, pc) and not k[2] and k[3] for k in c.items), (kind, pc, "luma clamped, chroma inside")
        assert {k[1] for k in c.items if k[0] == "lane"} == set(IC.PHASE_CLASSES)
    elif which == "phase_set":
        for kind in ("mb", "quad", "lane"):
            assert {(k[1], k[2]) for k in c.cells if k[0] == "c" and k[3] == kind} == {(x, y) for x in range(8) for y in range(8)}, kind
            assert {(k[1], k[2]) for k in c.cells if k[0] == "y" and k[3] == kind} == set(every), kind
    elif which == "shape_set":
        assert set(stims[0].pic.shapes.values()) == set(SHAPES)
        assert {(st.pic.mb_w, st.pic.mb_h) for st in stims} == {(MB_W, MB_H), (2, 18), (11, 1), (1, 9)}
        assert {k[3] for k in c.cells} == {"mb", "quad", "lane"}
    elif which == "b_set":
        assert {k for k in c.roads if isinstance(k, tuple)} == {(r, w) for r in IC.B_ROADS for w in (0, 1)}, sorted(c.roads, key=str)
        assert {w for f, w in c.weights if f} >= set(B_WEIGHTS) and min(B_WEIGHTS) < 0 and 128 in B_WEIGHTS and (0, 32) in c.weights
        for lists in ("l0", "l1", "bi"):
            assert any(k[5] == lists and "past" in k[4] for k in c.cells) and any(k[5] == lists and k[6] for k in c.cells), lists
    elif which == "limit_set":
        xs, ys = set(), set()
        for st in stims:
            mv = st.pic.mv.reshape(-1, 2)
            xs |= set(mv[:, 0].tolist())
            ys |= set(mv[:, 1].tolist())
            assert mv[:, 0].min() >= -8192 and mv[:, 0].max() <= 8191 and mv[:, 1].min() >= -2048 and mv[:, 1].max() <= 2047
        assert xs >= set(LIMITS_X) and ys >= set(LIMITS_Y)
        for kind in ("mb", "quad", "lane"):
            for side in range(4):
                assert "out" in {k[4][side] for k in c.cells if k[3] == kind}, (kind, side)
    elif which == "weighted_set":
        assert c.roads["wp"] > 30 and {k[5] for k in c.cells} == {"l0", "l1", "bi"}
        assert {st.pic.desc.slice_type for st in stims} == {N.SLICE_P, N.SLICE_B} and all(st.pic.desc.explicit_wp for st in stims)
    else:
        assert which == "residual_set", which
        assert {st.pic.desc.chroma_qp_offset for st in stims} == set(range(-12, 13))
        seen = new_residual_survey()
        for st in stims:
            residual_survey(st.pic, seen)
        for name, cells in residual_cells().items():
            assert not cells - seen[name], "%s: not reached: %s" % (name, sorted(cells - seen[name], key=str)[:10])
        # the two DC branches' rounding rules show in few samples: blocks that tell, held to a count
        assert seen["tells"]["luma DC rounded"] >= 100 and seen["tells"]["chroma DC truncated"] >= 40, seen["tells"]
        assert coded > 1500 and changed > 0
    return c
