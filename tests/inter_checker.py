"""Checker for inter prediction (TEST INFRASTRUCTURE), written from the text of H.264 8.4.2.2 / 8.4.2.3 - not from
oracle/cpu_recon.c (oracle_mc_luma / oracle_mc_chroma restate the reference's four half-sample planes, its quarter-sample
average and its "correction" bit), not from kernel_mc.h and not from the reference.  Plain numpy integers (int64); nothing of the
oracle is called or loaded.

* luma, 8.4.2.2.1: the full samples G, H, M (and their neighbours) are read at Clip3(0, W - 1, x), Clip3(0, H - 1, y)
  (eq. 8-229 / 8-230); b1, h1 (and s1, m1: the same filter one row down / one column right) from the 6-tap filter, b = Clip1((b1 +
  16) >> 5); j1 from the unclipped intermediates, j = Clip1((j1 + 512) >> 10); the sixteen positions by TABLE 8-12, each an entry
  of `LUMA_POSITIONS` addressed by (xFrac, yFrac): a sample, or the average (p + q + 1) >> 1 of two named samples.
* chroma, 8.4.2.2.2: ((8 - xF)(8 - yF) A + xF (8 - yF) B + (8 - xF) yF C + xF yF D + 32) >> 6 with the luma vector taken in units
  of one eighth chroma sample (frame pictures, 4:2:0: the chroma vector equals the luma vector).
* the lists, include/p264hip.h: an index at or past its list means entry 0; a quadrant with no list at all uses list 0, entry 0.
  One list: the prediction itself.  Two lists: weighted_bipred == 0 -> (p0 + p1 + 1) >> 1 (8.4.2.3.1); != 0 -> 8.4.2.3.2 with
  logWD 5, offsets 0, w0 = bipred_weight[entry0 * 16 + entry1], w1 = 64 - w0.  explicit_wp: wp_checker._weigh (8.4.2.3.2).

`predict(pic, frames, census)` writes the prediction of every inter macroblock into the picture's frame.  The census (a `Census`)
records per predicted 4x4 block, list and plane the cell (plane, xFrac, yFrac, item kind, the four sides of the item's read
window, lists used) and counts the j intermediates outside -80 .. 335 (the domain of the reference's clip table, SURVEY A-Q13:
reported, never excluded - the standard's Clip1 is what is computed).  The item kind and the window are those of kernel_mc.h's
mc_classify, restated from its description: a macroblock with one vector and one reference is ONE item ('mb': luma window 21 x 21
at (16 mbx + (mvx >> 2) - 2, ...), chroma 9 x 9 at (8 mbx + (mvx >> 3), ...)); else each 8x8 quadrant with one vector is an item
('quad': 13 x 13, 5 x 5); a quadrant whose 4x4 blocks differ - and every block of a two-list macroblock with such a quadrant, and
every block of a picture with explicit weights - is fetched per block ('lane': 9 x 9, 3 x 3)."""
import collections

import numpy as np

from p264decoder_amd import _native as N

PHASE_CLASSES = ("copy", "h", "v", "diag", "c", "ch", "cv")
B_ROADS = ("list0 only", "list1 only", "generic", "second pass whole", "second pass quadrants", "second pass with carried quadrants")
# table 8-12: (xFrac, yFrac) -> the predicted sample: a name of figure 8-4, or the two names whose average it is
LUMA_POSITIONS = {
    (0, 0): ("G",), (0, 1): ("G", "h"), (0, 2): ("h",), (0, 3): ("M", "h"),
    (1, 0): ("G", "b"), (1, 1): ("b", "h"), (1, 2): ("h", "j"), (1, 3): ("h", "s"),
    (2, 0): ("b",), (2, 1): ("b", "j"), (2, 2): ("j",), (2, 3): ("j", "s"),
    (3, 0): ("H", "b"), (3, 1): ("b", "m"), (3, 2): ("j", "m"), (3, 3): ("m", "s"),
}


def window(plane, x0, y0, w, h):
    """the w x h samples from (x0, y0), each read at Clip3(0, W - 1, x), Clip3(0, H - 1, y)"""
    H, W = plane.shape
    ys = np.clip(np.arange(y0, y0 + h), 0, H - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, W - 1)
    return plane[np.ix_(ys, xs)].astype(np.int64)


def _tap(a, b, c, d, e, f):
    return a - 5 * b + 20 * c + 20 * d - 5 * e + f


def _clip1(v):
    return np.clip(v, 0, 255)


def luma_block(plane, x_int, y_int, x_frac, y_frac, n=4, stats=None):
    """8.4.2.2.1 for the n x n samples whose full-sample location is (x_int, y_int) + (0 .. n - 1): int64[n][n]"""
    S = window(plane, x_int - 2, y_int - 2, n + 6, n + 6)          # S[r + 2][c + 2] = the full sample at (x_int + c, y_int + r)
    names = LUMA_POSITIONS[(x_frac, y_frac)]
    v = {}
    v["G"] = S[2:2 + n, 2:2 + n]
    v["H"] = S[2:2 + n, 3:3 + n]
    v["M"] = S[3:3 + n, 2:2 + n]
    if set(names) & set("bsj"):
        # b1 at (row r, column c) for r = -2 .. n + 3, c = 0 .. n - 1: E, F, G, H, I, J of that row
        b1 = _tap(S[:, 0:n], S[:, 1:1 + n], S[:, 2:2 + n], S[:, 3:3 + n], S[:, 4:4 + n], S[:, 5:5 + n])
        b = _clip1((b1 + 16) >> 5)
        v["b"] = b[2:2 + n]
        v["s"] = b[3:3 + n]                                         # the same filter one row down (between M and N)
        if "j" in names:
            j = (_tap(b1[0:n], b1[1:1 + n], b1[2:2 + n], b1[3:3 + n], b1[4:4 + n], b1[5:5 + n]) + 512) >> 10
            if stats is not None:
                stats["j"] += j.size
                stats["j_outside"] += int(((j < -80) | (j > 335)).sum())
            v["j"] = _clip1(j)
    if set(names) & set("hm"):
        h1 = _tap(S[0:n, :], S[1:1 + n, :], S[2:2 + n, :], S[3:3 + n, :], S[4:4 + n, :], S[5:5 + n, :])
        h = _clip1((h1 + 16) >> 5)
        v["h"] = h[:, 2:2 + n]
        v["m"] = h[:, 3:3 + n]                                      # the same filter one column right (between H and N)
    if len(names) == 1:
        return v[names[0]].copy()
    return (v[names[0]] + v[names[1]] + 1) >> 1


def chroma_block(plane, x_int, y_int, x_frac, y_frac, n=2):
    """8.4.2.2.2 for n x n chroma samples: (x_int, y_int) the location of A, fractions in eighths"""
    S = window(plane, x_int, y_int, n + 1, n + 1)
    A, B, C_, D = S[:n, :n], S[:n, 1:], S[1:, :n], S[1:, 1:]
    return ((8 - x_frac) * (8 - y_frac) * A + x_frac * (8 - y_frac) * B + (8 - x_frac) * y_frac * C_ + x_frac * y_frac * D + 32) >> 6


def phase_class(fx, fy):
    """which arithmetic a luma vector's fractions need (the classes k_mc sorts its work by)"""
    if fx == 0 and fy == 0:
        return "copy"
    if fy == 0:
        return "h"
    if fx == 0:
        return "v"
    if fx & fy & 1:
        return "diag"
    if fx == 2:
        return "c" if fy == 2 else "ch"
    return "cv"


# ---- which lists, which entries --------------------------------------------------------------------------------------------
def quadrant_lists(pic, m, q):
    """(use0, use1, entry0, entry1) of quadrant q of inter macroblock m"""
    d = pic.desc
    r0 = int(pic.ref_idx[m * 4 + q])
    r1 = int(pic.ref_idx_l1[m * 4 + q]) if d.slice_type == N.SLICE_B else -1
    use1 = r1 >= 0
    use0 = r0 >= 0 or not use1
    return use0, use1, (r0 if 0 <= r0 < d.n_ref else 0), (r1 if use1 and r1 < d.n_ref_l1 else 0)


def _vec(a, m, b):
    return int(a[(m * 16 + b) * 2]), int(a[(m * 16 + b) * 2 + 1])


def _quad_blocks(q):
    b0 = (q >> 1) * 8 + (q & 1) * 2
    return (b0, b0 + 1, b0 + 4, b0 + 5)


quad_blocks = _quad_blocks             # (public names: tests/worklist_model.py and tests/worklist_stim.py build on them)


def classify(pic, m):
    """The work items inter macroblock m becomes: {(list, block): (kind, blocks of the item, (mvx, mvy) of the item or None)} for
    every (list, 4x4 block in raster order) that is predicted - kind 'mb' / 'quad' / 'lane' as in the module's text - and the
    road through the stage (one of B_ROADS, 'p' for a macroblock of a P picture, 'wp' under explicit weights)."""
    d = pic.desc
    is_b = d.slice_type == N.SLICE_B
    L = [quadrant_lists(pic, m, q) for q in range(4)]
    vecs = [[_vec(pic.mv, m, b) for b in range(16)], [_vec(pic.mv_l1, m, b) for b in range(16)] if is_b else [(0, 0)] * 16]
    out = {}

    def uniform(l, q):
        return len({vecs[l][b] for b in _quad_blocks(q)}) == 1

    def lanes(road):
        for q in range(4):
            for l in (0, 1):
                if L[q][l]:
                    for b in _quad_blocks(q):
                        out[(l, b)] = ("lane", (b,), None)
        return out, road

    if d.explicit_wp:
        return lanes("wp")
    two = is_b and any(u1 or not (int(pic.ref_idx[m * 4 + q]) >= 0) for q, (u0, u1, e0, e1) in enumerate(L))
    if two and not all((not L[q][l]) or uniform(l, q) for q in range(4) for l in (0, 1)):
        return lanes("generic")
    passes = []
    if not two:
        passes.append([(0, L[q][2], vecs[0][_quad_blocks(q)[0]] if uniform(0, q) else None, False) for q in range(4)])
        road = "list0 only" if is_b else "p"
    else:
        first, second = [], []
        for q, (u0, u1, e0, e1) in enumerate(L):
            bi = u0 and u1
            l = 0 if u0 else 1
            first.append((l, (e0, e1)[l], vecs[l][_quad_blocks(q)[0]], bi))
            # (the second pass keeps list-0 indices apart as coded: the weight belongs to the pair)
            second.append((1, (int(pic.ref_idx[m * 4 + q]) & 15, e1), vecs[1][_quad_blocks(q)[0]], False) if bi else None)
        passes.append(first)
        n_bi = sum(s is not None for s in second)
        if n_bi:
            passes.append(second)
        road = ("list1 only" if n_bi == 0 else "second pass with carried quadrants" if n_bi < 4 else
                "second pass whole" if len(set(second)) == 1 else "second pass quadrants")
    for items in passes:
        if all(i is not None for i in items) and len(set(items)) == 1 and items[0][2] is not None:
            for b in range(16):
                out[(items[0][0], b)] = ("mb", tuple(range(16)), items[0][2])
            continue
        for q, it in enumerate(items):
            if it is None:
                continue
            for b in _quad_blocks(q):
                out[(it[0], b)] = ("quad", _quad_blocks(q), it[2]) if it[2] is not None else ("lane", (b,), None)
    return out, road


def _side(lo, n, size):
    """the two sides of a window of n samples from lo in a dimension of `size`: 'in', 'flush' (ends exactly at the border), 'past'
    (reaches over it), 'out' (the whole window lies beyond it)"""
    hi = lo + n
    a = "out" if hi <= 0 else "past" if lo < 0 else "flush" if lo == 0 else "in"
    b = "out" if lo >= size else "past" if hi > size else "flush" if hi == size else "in"
    return a, b


side = _side


DECODE_INDEX = {bb: i for i, bb in enumerate([0, 1, 4, 5, 2, 3, 6, 7, 8, 9, 12, 13, 10, 11, 14, 15])}     # raster 4x4 block -> coef_mask bit
LUMA_WINDOW = {"mb": (21, 16), "quad": (13, 8), "lane": (9, 4)}       # kind -> (window, item) size in samples
CHROMA_WINDOW = {"mb": (9, 8), "quad": (5, 4), "lane": (3, 2)}


def item_window(pic, m, kind, blocks, vec, chroma):
    """(x, y, n) of the item's read window (the module's text) in the plane"""
    b = blocks[0]
    x0, y0 = (m % pic.mb_w) * 16 + (b & 3) * 4, (m // pic.mb_w) * 16 + (b >> 2) * 4
    if chroma:
        return x0 // 2 + (vec[0] >> 3), y0 // 2 + (vec[1] >> 3), CHROMA_WINDOW[kind][0]
    return x0 + (vec[0] >> 2) - 2, y0 + (vec[1] >> 2) - 2, LUMA_WINDOW[kind][0]


class Census:
    """cells: Counter of (plane 'y' / 'c', xFrac, yFrac, kind, (left, right, top, bottom), lists 'l0' / 'l1' / 'bi', coded) per
    predicted 4x4 block, list and plane kind - coded: the plane's residual of the block's ITEM is present (the RESID bit of the
    item's key: any luma block of the item / any chroma level of the macroblock); items: Counter of (kind, phase class, luma window
    inside, chroma window inside, luma coded, chroma coded) per luma item; roads: Counter of classify's roads - (road, weighted_bipred) for the macroblocks of B pictures without explicit weights; weights: the set of
    (weighted_bipred, w0) of the bi-predicted blocks; stats: j / j_outside; entries: Counter of (list, entry, item kind, 'p' / 'b'
    by the picture's slice type, road) per predicted 4x4 block and list; pairs: Counter of (entry 0, entry 1, item kind of the
    list-0 fetch, road) per bi-predicted 4x4 block."""

    def __init__(self):
        self.cells = collections.Counter()
        self.items = collections.Counter()
        self.roads = collections.Counter()
        self.weights = set()
        self.stats = collections.Counter()
        self.entries = collections.Counter()
        self.pairs = collections.Counter()


def _inside(sides):
    return all(s in ("in", "flush") for s in sides)


inside = _inside


def survey(pic, census):
    """what the picture's inter macroblocks exercise, from its arrays alone (no sample is read)"""
    d = pic.desc
    rec = pic.mb_records()
    W, H = d.mb_w * 16, d.mb_h * 16
    for m in np.flatnonzero(rec["mb_type"] > N.MB_IPCM):
        m = int(m)
        items, road = classify(pic, m)
        census.roads[(road, int(d.weighted_bipred)) if road in B_ROADS else road] += 1
        mask = int(rec["coef_mask"][m])
        cc = bool(mask & (0x00ff0000 | N.COEF_CHROMA_DC))
        seen = set()
        for (l, b), (kind, blocks, vec) in sorted(items.items()):
            q = (b >> 3) * 2 + ((b & 3) >> 1)
            u0, u1, e0, e1 = quadrant_lists(pic, m, q)
            lists = "bi" if u0 and u1 else "l1" if u1 else "l0"
            v = vec if vec is not None else _vec(pic.mv_l1 if l else pic.mv, m, b)
            first_of_two = lists == "bi" and l == 0 and road.startswith("second pass")     # the second pass adds the residual
            # (the residual bit of a per-block fetch's key is its quadrant's)
            coded_y = any(mask >> DECODE_INDEX[bb] & 1 for bb in (_quad_blocks(q) if kind == "lane" else blocks)) and not first_of_two
            coded_c = cc and not first_of_two
            sy, sc = [], []
            for chroma, acc in ((False, sy), (True, sc)):
                x, y, n = item_window(pic, m, kind, blocks, v, chroma)
                acc += _side(x, n, W >> chroma) + _side(y, n, H >> chroma)
            census.cells[("y", v[0] & 3, v[1] & 3, kind, tuple(sy), lists, coded_y)] += 1
            census.cells[("c", v[0] & 7, v[1] & 7, kind, tuple(sc), lists, coded_c)] += 1
            census.entries[(l, (e0, e1)[l], kind, "b" if d.slice_type == N.SLICE_B else "p", road)] += 1
            if lists == "bi" and l == 0:
                census.pairs[(e0, e1, kind, road)] += 1
            if (l, blocks) not in seen:
                seen.add((l, blocks))
                census.items[(kind, phase_class(v[0] & 3, v[1] & 3), _inside(sy), _inside(sc), coded_y, coded_c)] += 1
            if lists == "bi" and l == 0 and not d.explicit_wp:
                census.weights.add((int(d.weighted_bipred), int(d.bipred_weight[e0 * N.MAX_REFS + e1]) if d.weighted_bipred else 32))
    return census


# ---- the prediction of a picture --------------------------------------------------------------------------------------------
def combine(pic, p0, p1, e0, e1, plane):
    """8.4.2.3 for one block: p0 / p1 int64 arrays or None (list unused)"""
    d = pic.desc
    if d.explicit_wp:
        from tests.wp_checker import _weigh
        tab = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2).astype(np.int64)
        return _weigh(p0, p1, p0 is not None, p1 is not None, tab[0, e0, plane], tab[1, e1, plane], int(d.wp_log2_denom[min(plane, 1)]))
    if p0 is None or p1 is None:
        return p0 if p1 is None else p1
    if not d.weighted_bipred:
        return (p0 + p1 + 1) >> 1                                    # 8.4.2.3.1
    w0 = int(d.bipred_weight[e0 * N.MAX_REFS + e1])
    return _clip1((p0 * w0 + p1 * (64 - w0) + 32) >> 6)              # 8.4.2.3.2: logWD = 5, o0 = o1 = 0, w1 = 64 - w0


def predict(pic, frames, census=None):
    """the inter prediction samples of every inter macroblock of pic, written into frames[dst_slot] (frames[slot] = [y, u, v]
    uint8 arrays); the census, if given, also takes the picture's survey"""
    d = pic.desc
    rec = pic.mb_records()
    F = frames[d.dst_slot]
    stats = census.stats if census is not None else None
    if census is not None:
        survey(pic, census)
    for m in np.flatnonzero(rec["mb_type"] > N.MB_IPCM):
        m = int(m)
        mbx, mby = m % d.mb_w, m // d.mb_w
        # (a sample depends only on its own block's vector and lists: blocks that share them are predicted in one piece - a
        # quadrant of 8 x 8, a macroblock of 16 x 16 - which is the same samples in fewer numpy calls)
        units = []
        for q in range(4):
            lists = quadrant_lists(pic, m, q)
            qb = _quad_blocks(q)
            vs = [(_vec(pic.mv, m, b) if lists[0] else (0, 0), _vec(pic.mv_l1, m, b) if lists[1] else (0, 0)) for b in qb]
            if len(set(vs)) == 1:
                units.append((qb[0], 8, vs[0], lists))
            else:
                units += [(b, 4, v, lists) for b, v in zip(qb, vs)]
        if len(units) == 4 and len({u[1:] for u in units}) == 1:
            units = [(0, 16, units[0][2], units[0][3])]
        for b, n, (v0, v1), (use0, use1, e0, e1) in units:
            X, Y = mbx * 16 + (b & 3) * 4, mby * 16 + (b >> 2) * 4
            for plane in range(3):
                p = [None, None]
                for l, (use, e, v) in enumerate(((use0, e0, v0), (use1, e1, v1))):
                    if not use:
                        continue
                    src = frames[int(d.ref_slot_l1[e] if l else d.ref_slot[e])][plane]
                    if plane == 0:
                        p[l] = luma_block(src, X + (v[0] >> 2), Y + (v[1] >> 2), v[0] & 3, v[1] & 3, n, stats)
                    else:
                        p[l] = chroma_block(src, X // 2 + (v[0] >> 3), Y // 2 + (v[1] >> 3), v[0] & 7, v[1] & 7, n // 2)
                o = combine(pic, p[0], p[1], e0, e1, plane)
                if plane == 0:
                    F[0][Y:Y + n, X:X + n] = o
                else:
                    F[plane][Y // 2:Y // 2 + n // 2, X // 2:X // 2 + n // 2] = o
    return F
