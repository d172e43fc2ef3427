"""Directed pictures for the loop filter (TEST INFRASTRUCTURE): pictures at the CPU->GPU seam whose lines across the edges are
DRAWN PER CELL of tests/deblock_checker.py's census - rejection sampling of p3..q3 against the alpha / beta / tc0 the edge's QPs
and the picture's offsets give - instead of hoping that random content reaches the filter's rare branches.

How chosen samples get either side of an edge of a chosen strength without touching them:

* strengths 1 and 2 ("inter" pictures): every macroblock is an inter macroblock with vector 0 and no levels, so the unfiltered
  picture IS the reference frame, which the builder writes.  Strength 1: the quadrants' indices alternate between two list
  entries that live in DIFFERENT frame-store slots with equal contents (different reference pictures, 8.7.2.1) - across the
  macroblock edge and across inner edge 2 of the focused direction, 0 in the other direction.  Strength 2: block column 0 or
  block columns 0 and 2 carry coded blocks whose levels are all zero.  The focused edges are 0 and 2, whose eight-sample lines
  tile a row; p3 and q3, which no filter of strength < 4 reads, are set to 255 / 0 so that the edges in between (1 and 3) fail
  |p0 - q0| < alpha and leave the drawn lines alone.
* strengths 3 and 4 ("intra" pictures): rows of inter macroblocks that copy drawn content alternate with rows in which every
  second macroblock is Intra16x16 with vertical prediction (chroma too) and no levels: it repeats the row above - drawn - down
  its sixteen lines, so the samples across its inner vertical edges (strength 3) are that row's; across its left edge (strength
  4) lie sixteen different drawn lines of the inter macroblock to its left and the row's first four samples, across the left
  edge of the inter macroblock to its right the row's last four and sixteen drawn lines.  Prediction reads unfiltered samples, so
  the filter's own writes do not disturb the construction.
* horizontal edges: the same construction transposed (macroblock grid, content, coded blocks, quadrants; horizontal prediction).

QPs: every row of macroblocks (column, when transposed) takes the QP that puts indexA of the plane it is meant for at the next
value of SWEEP - 0 .. 51 with 15 / 16 / 17 (alpha 0 -> 4 while tc0 is still 0), 20 / 21, 22 / 23 / 24 and 51 - every second
macroblock 2 above it, so that macroblock edges see the mean of two QPs.  Offsets -12 .. 12, odd and even; chroma_qp_offset -12 .. 12.

What in-place filtering does to a drawn line (an earlier edge of the same macroblock changed some of its samples, the vertical
pass ran before the horizontal one) is not modelled: the census of the checker's own run counts what it met, and
tests/test_deblock_checker_cpu.py holds it to at least 8 lines in every cell.  Everything is generated from seeds; nothing is data."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import deblock_checker as D
from tests import oracle_bind, seam_fuzz

MB_W, MB_H = 9, 6            # v-space grid (transposed pictures are 6 x 9): lines cross octets, bands of 4 rows and the ring
SWEEP = [16, 17, 23, 40, 16, 20, 24, 51, 8, 16, 21, 30, 46, 15, 16, 22, 36, 19, 16, 28, 0, 18, 16, 33, 43, 12, 16, 26, 49, 38]
Stim = collections.namedtuple("Stim", "name pic frame ref_slots")   # frame: the [y, u, v] every slot of ref_slots holds


def _g(rng, beta):
    k = int(rng.integers(0, 3))
    w = 2 if k == 0 else beta // 2 + 1 if k == 1 else beta + 2
    return int(rng.integers(-w, w + 1))


def candidate(rng, chroma, alpha, beta, fixed_p=None, fixed_q=None, base=None):
    """one candidate line: a base anywhere, near 0 or near 255; a step across the edge around the interesting sizes (0, the strong
    filter's (alpha >> 2) + 2, alpha); gradients inside either side around beta.  fixed_p / fixed_q: that side is given; base: 2 / 3
    = p0 near 0 / near 255."""
    steps = (0, 1, 2, 3, (alpha >> 2) + 1, (alpha >> 2) + 2, (alpha >> 2) + 3, alpha - 1, alpha, alpha + 1, int(rng.integers(0, alpha + 2)), 8 * beta)
    d0 = int(steps[int(rng.integers(0, len(steps)))]) * (1 if rng.random() < 0.5 else -1)
    n = 2 if chroma else 4
    if fixed_p is not None:
        p0 = fixed_p[-1]
    elif fixed_q is not None:
        p0 = fixed_q[0] - d0
    else:
        k = int(rng.integers(0, 4)) if base is None else base
        p0 = int(rng.integers(0, 256)) if k < 2 else int(rng.integers(0, 8)) if k == 2 else int(rng.integers(248, 256))
    q0 = fixed_q[0] if fixed_q is not None else p0 + d0

    def side(x0):
        out = [x0, x0 + _g(rng, beta)]
        if n == 4:
            # (p2 / q2: a third of them at beta .. beta + 2 from p0 / q0, either way - where ap / aq < beta turns)
            out.append(x0 + (_g(rng, beta) if rng.random() < 0.67 else (beta + int(rng.integers(0, 3))) * (1 if rng.random() < 0.5 else -1)))
            out.append(out[2] + _g(rng, beta))
        return [min(max(v, 0), 255) for v in out]
    p = list(fixed_p) if fixed_p is not None else side(p0)[::-1]
    q = list(fixed_q) if fixed_q is not None else side(q0)
    return p + q


def draw_line(rng, chroma, bs, cl, ia, alpha, beta, fixed_p=None, fixed_q=None, tries=100):
    """a line of class cl, or None"""
    if cl.startswith("off/"):
        if (cl == "off/alpha=0") != (alpha == 0):
            return None
    elif alpha == 0 or beta == 0:
        return None
    elif cl.startswith("delta") and cl.endswith("tc0=0") != (D.TC0[ia][bs - 1] == 0):
        return None
    base = 2 if cl == "clipped at 0" else 3 if cl == "clipped at 255" else None       # (Clip1 needs samples next to 0 / 255)
    if base is not None or cl == "delta saturates/tc0=0":                              # (the rare ones: see OFFSETS_INTRA)
        tries *= 6
    hits = []
    for _ in range(tries):
        s = candidate(rng, chroma, alpha, beta, fixed_p, fixed_q, base)
        del hits[:]
        D.filter_line(s, chroma, bs, ia, alpha, beta, hits)
        if cl in hits:
            return s
    return None


CAP = 24                     # lines aimed at a cell before the builder stops aiming at it (the condition is 8 lines met)


class _Need:
    """how often each cell has been aimed at: the next line goes for the cell that has been aimed at least, until every cell the
    edge can reach has been aimed at CAP times; parameter sets at which a class was not found are remembered"""

    def __init__(self):
        self.aimed = collections.Counter()
        self.failed = collections.Counter()

    def line(self, rng, chroma, bs, dr, parities, where, ia, alpha, beta, fixed_p=None, fixed_q=None, weight=1):
        plane = "c" if chroma else "y"
        free = fixed_p is None and fixed_q is None
        key = (chroma, bs, ia, alpha, beta, free)
        classes = [c for c in D.line_classes(chroma, bs) if (plane, bs, c) not in D.IMPOSSIBLE
                   and self.aimed[(plane, bs, c, dr, parities[0], where)] < CAP and self.failed[key + (c,)] < (2 if free else 3)]
        order = sorted(classes, key=lambda c: (self.aimed[(plane, bs, c, dr, parities[0], where)], rng.random()))
        for cl in order[:3]:
            s = draw_line(rng, chroma, bs, cl, ia, alpha, beta, fixed_p, fixed_q)
            if s is not None:
                for par in parities:
                    self.aimed[(plane, bs, cl, dr, par, where)] += weight
                return s
            self.failed[key + (cl,)] += 1
        return candidate(rng, chroma, alpha, beta, fixed_p, fixed_q)


def _qp_for(ia_want, off_a, chroma, cqo):
    """the QP whose indexA (of the luma or chroma plane) is closest to ia_want"""
    def ia_of(q):
        return (D.chroma_qp_av(q, q, cqo) if chroma else q) + off_a
    return min(range(52), key=lambda q: (abs(ia_of(q) - ia_want), q))


class _Builder:
    """a picture in v-space: focused edges are vertical; emit(transpose) gives the seam picture and its reference frame"""

    def __init__(self, rng, need, dr, offsets):
        self.rng, self.need, self.dr = rng, need, dr
        self.off_a, self.off_b, self.cqo = offsets
        self.Y = rng.integers(0, 256, size=(MB_H * 16, MB_W * 16)).astype(np.int64)
        self.C = [rng.integers(0, 256, size=(MB_H * 8, MB_W * 8)).astype(np.int64) for _ in range(2)]
        self.qp = np.zeros((MB_H, MB_W), np.int64)
        self.kind = np.zeros((MB_H, MB_W), np.int64)            # 0 inter, 1 Intra16x16 vertical
        self.refs = np.zeros((MB_H, MB_W, 4), np.int64)         # list-0 index per quadrant
        self.coded = np.zeros((MB_H, MB_W, 4, 4), bool)         # [block y][block x]

    def set_qps(self, sweep_at, intra=False):
        for r in range(MB_H):
            chroma = (sweep_at + r) % 3 == 2                    # two rows in three aim indexA at luma, one at chroma
            want = SWEEP[(sweep_at + r) % len(SWEEP)]
            if intra and r == 1:                                # strength 3 has tc0 = 0 at indexA 16 alone (table 8-17): one row per picture
                want, chroma = 16, bool(sweep_at & 1)
            q = _qp_for(want, self.off_a, chroma, self.cqo)
            if intra and r == 1 and chroma and D.chroma_qp_av(q, q, self.cqo) + self.off_a != 16:
                q = _qp_for(want, self.off_a, False, self.cqo)  # (no QP puts the chroma planes there with these offsets: luma then)
            for c in range(MB_W):
                self.qp[r, c] = min(q + 2 * (c & 1) * ((r >> 1) & 1), 51)      # rows 2, 3: every second macroblock 2 above

    def params(self, r, cp, cq, chroma):
        qp_av = D.chroma_qp_av(int(self.qp[r, cp]), int(self.qp[r, cq]), self.cqo) if chroma else (int(self.qp[r, cp]) + int(self.qp[r, cq]) + 1) >> 1
        return D.thresholds(qp_av, self.off_a, self.off_b)

    # ---- strengths 1 and 2 ----
    def inter_picture(self, bs):
        rng = self.rng
        for r in range(MB_H):
            for c in range(MB_W):
                if bs == 1:
                    self.refs[r, c] = [0, 1, 0, 1]
                else:
                    self.coded[r, c, :, 0] = True
                    self.coded[r, c, :, 2] = True
                for chroma in (False, True):
                    size, half = (8, 2) if chroma else (16, 4)
                    for e in (0, 2):
                        if e == 0 and c == 0:
                            continue
                        ia, alpha, beta = self.params(r, c - 1 if e == 0 else c, c, chroma)
                        x = c * size + e * size // 4 - half
                        for P in (self.C if chroma else [self.Y]):
                            for k in range(size):
                                s = self.need.line(rng, chroma, bs, self.dr, (k & 1,), "inner" if e else "mb", ia, alpha, beta)
                                if not chroma:
                                    s[0], s[7] = 0, 255        # p3 / q3: unread at strengths < 4; edges 1 and 3 see |255 - 0| >= alpha
                                P[r * size + k, x:x + 2 * half] = s

    # ---- strengths 3 and 4 ----
    def intra_picture(self):
        rng = self.rng
        for r in range(1, MB_H, 2):
            for c in range(1, MB_W - 1, 2):
                self.kind[r, c] = 1
                for chroma in (False, True):
                    size, half = (8, 2) if chroma else (16, 4)
                    for P in (self.C if chroma else [self.Y]):
                        y0, x0 = r * size, c * size
                        row = P[y0 - 1]                         # the bottom row of the macroblock above: what vertical prediction repeats
                        # the last inner edge (luma edge 3, chroma edge 2): strength 3, sixteen (eight) equal lines
                        ia, alpha, beta = self.params(r, c, c, chroma)
                        at = x0 + (12 if not chroma else 4) - half
                        s3 = self.need.line(rng, chroma, 3, self.dr, (0, 1), "inner", ia, alpha, beta, weight=size // 2)
                        if not chroma:
                            s3[0] = 255                         # (p3: unread; luma edge 2 sees |s[7] - 255| below)
                        row[at:at + 2 * half] = s3
                        after = D.filter_line(list(s3), chroma, 3, ia, alpha, beta)
                        # the left edge: strength 4; q = the row's first samples, p = a line of the inter macroblock to the left
                        ia, alpha, beta = self.params(r, c - 1, c, chroma)
                        first = self.need.line(rng, chroma, 4, self.dr, (0,), "mb", ia, alpha, beta)
                        row[x0:x0 + half] = first[half:]
                        P[y0, x0 - half:x0] = first[:half]
                        for k in range(1, size):
                            s = self.need.line(rng, chroma, 4, self.dr, (k & 1,), "mb", ia, alpha, beta, fixed_q=first[half:])
                            P[y0 + k, x0 - half:x0] = s[:half]
                        if not chroma:
                            # luma edge 1: strength 3, p given (and about to be changed by the left edge: a by-product); its q3 = 0
                            ia, alpha, beta = self.params(r, c, c, chroma)
                            s1 = self.need.line(rng, chroma, 3, self.dr, (0, 1), "inner", ia, alpha, beta, fixed_p=[int(v) for v in row[x0:x0 + 4]], weight=0)
                            s1[7] = 0
                            row[x0 + 4:x0 + 8] = s1[4:]
                        # the left edge of the inter macroblock to the right: strength 4; p = the row's last samples (luma: as edge 3
                        # left them; chroma: samples 6, 7 lie beyond the reach of edge 2 and are drawn with the first line)
                        ia, alpha, beta = self.params(r, c, c + 1, chroma)
                        if chroma:
                            s = self.need.line(rng, chroma, 4, self.dr, (0,), "mb", ia, alpha, beta)
                            row[x0 + 6:x0 + 8] = s[:half]
                            P[y0, x0 + size:x0 + size + half] = s[half:]
                            fp, rest = s[:half], range(1, size)
                        else:
                            fp, rest = [int(v) for v in after[half:]], range(size)
                        for k in rest:
                            s = self.need.line(rng, chroma, 4, self.dr, (k & 1,), "mb", ia, alpha, beta, fixed_p=fp)
                            P[y0 + k, x0 + size:x0 + size + half] = s[half:]

    # ---- the seam picture ----
    def emit(self, name, transpose, slots=3, dst_slot=0, ref_slots=(1, 2)):
        w, h = (MB_H, MB_W) if transpose else (MB_W, MB_H)
        pic = seam_fuzz.SeamPicture(w, h)
        d = pic.desc
        d.slice_type = N.SLICE_P
        d.chroma_qp_offset, d.alpha_c0_offset, d.beta_offset = self.cqo, self.off_a, self.off_b
        d.deblock, d.dst_slot, d.n_ref = 1, dst_slot, 2
        d.ref_slot[0], d.ref_slot[1] = ref_slots
        rec = pic.rec
        blocks = []
        for m in range(w * h):
            x, y = m % w, m // w
            r, c = (x, y) if transpose else (y, x)
            rr = rec[m]
            rr["qp"] = int(self.qp[r, c])
            rr["avail"] = (N.AVAIL_LEFT if x else 0) | (N.AVAIL_TOP if y else 0) | (N.AVAIL_TOPRIGHT if y and x + 1 < w else 0) | (N.AVAIL_TOPLEFT if x and y else 0)
            rr["edges"] = N.EDGE_INNER | (N.EDGE_LEFT if x else 0) | (N.EDGE_TOP if y else 0)
            rr["coef_index"] = len(blocks)
            if self.kind[r, c]:
                rr["mb_type"] = N.MB_I16x16
                rr["intra_modes"] = (1 | 1 << 4) if transpose else (0 | 2 << 4)      # luma: 0 vertical, 1 horizontal; chroma: 1 horizontal, 2 vertical
                pic.ref_idx[m * 4:m * 4 + 4] = -1
                continue
            q = self.refs[r, c]
            q = [q[0], q[2], q[1], q[3]] if transpose else list(q)
            pic.ref_idx[m * 4:m * 4 + 4] = q
            rr["mb_type"] = N.MB_P_L0 if len(set(q)) == 1 else N.MB_P_8x8
            coded = self.coded[r, c].T if transpose else self.coded[r, c]
            mask = 0
            for b in range(16):
                if coded[seam_fuzz.BLK_Y[b], seam_fuzz.BLK_X[b]]:
                    mask |= 1 << b
                    blocks.append(np.zeros(16, np.int16))                          # coded, every level zero
            rr["coef_mask"] = mask
            rr["cbp"] = sum(1 << g for g in range(4) if (mask >> (4 * g)) & 15)
        d.n_coef_blocks = len(blocks)
        if blocks:
            pic.coefs = np.concatenate(blocks).astype(np.int16)
        planes = [self.Y] + self.C
        frame = [np.ascontiguousarray((p.T if transpose else p).astype(np.uint8)) for p in planes]
        return Stim(name, pic.seal(), frame, tuple(ref_slots))


OFFSETS = [(0, 0), (-3, 2), (5, -4), (12, 12), (-12, -7), (7, 9), (-6, -12), (2, -1), (-9, 5), (11, -11), (4, 6), (-1, -2)]
# (intra pictures: beta offset >= alpha offset, so that beta > 0 where indexA is 16 - and mostly 3 above it: at indexA 16 alpha is 4,
# |p0 - q0| <= 3, and a chroma line's delta (3 * (q0 - p0) + (p1 - p0) + (q0 - q1) + 4) >> 3 passes tc = 1 only with beta >= 3)
OFFSETS_INTRA = [(0, 3), (-3, 2), (12, 12), (-12, -7), (7, 10), (-9, 5), (4, 6), (-6, -1), (1, 12), (-11, -8)]


def stimulus_set(seed=8700, rounds=6):
    """the pictures: per round and edge direction one picture of strength 1, one of strength 2 and two of strengths 3 / 4"""
    rng = np.random.default_rng(seed)
    need = _Need()
    out = []
    k = 0
    for rnd in range(rounds):
        for dr in "vh":
            for kind in ("bs1", "bs2", "intra", "intra"):
                off_a, off_b = OFFSETS_INTRA[(k + rnd) * 3 % len(OFFSETS_INTRA)] if kind == "intra" else OFFSETS[(k + rnd) * 5 % len(OFFSETS)]
                cqo = int(rng.integers(-12, 13))
                b = _Builder(rng, need, dr, (off_a, off_b, cqo))
                b.set_qps(7 * (k // 2) + k, kind == "intra")
                if kind == "intra":
                    b.intra_picture()
                else:
                    b.inter_picture(1 if kind == "bs1" else 2)
                out.append(b.emit("%s_%s_%d" % (kind, dr, k), transpose=(dr == "h")))
                k += 1
    return out


def tiled_1080p(stim, mb_w=120, mb_h=68):
    """one large picture of a stimulus picture's rows repeated: the records, indices and content of `stim` tiled over mb_w x mb_h
    macroblocks (tile borders become ordinary edges between the tile's last and first macroblocks)"""
    src = stim.pic
    pic = seam_fuzz.SeamPicture(mb_w, mb_h)
    d, sd = pic.desc, src.desc
    d.slice_type, d.chroma_qp_offset, d.alpha_c0_offset, d.beta_offset = sd.slice_type, sd.chroma_qp_offset, sd.alpha_c0_offset, sd.beta_offset
    d.deblock, d.dst_slot, d.n_ref = 1, sd.dst_slot, sd.n_ref
    d.ref_slot[0], d.ref_slot[1] = sd.ref_slot[0], sd.ref_slot[1]
    blocks = []
    for m in range(mb_w * mb_h):
        x, y = m % mb_w, m // mb_w
        sm = (y % src.mb_h) * src.mb_w + x % src.mb_w
        pic.rec[m] = src.rec[sm]
        r = pic.rec[m]
        r["avail"] = (N.AVAIL_LEFT if x else 0) | (N.AVAIL_TOP if y else 0) | (N.AVAIL_TOPRIGHT if y and x + 1 < mb_w else 0) | (N.AVAIL_TOPLEFT if x and y else 0)
        r["edges"] = N.EDGE_INNER | (N.EDGE_LEFT if x else 0) | (N.EDGE_TOP if y else 0)
        if r["mb_type"] == N.MB_I16x16 and ((int(r["intra_modes"]) & 3) == 0 and y == 0 or (int(r["intra_modes"]) & 3) == 1 and x == 0):
            r["intra_modes"] = 2                                 # (no neighbour to predict from on the border: DC)
        pic.ref_idx[m * 4:m * 4 + 4] = src.ref_idx[sm * 4:sm * 4 + 4]
        r["coef_index"] = len(blocks)
        blocks += [np.zeros(16, np.int16)] * bin(int(r["coef_mask"]) & 0xffff).count("1")
    d.n_coef_blocks = len(blocks)
    if blocks:
        pic.coefs = np.concatenate(blocks).astype(np.int16)
    frame = []
    for p, s in zip(stim.frame, (16, 8, 8)):
        reps = (-(-mb_h * s // p.shape[0]), -(-mb_w * s // p.shape[1]))
        frame.append(np.ascontiguousarray(np.tile(p, reps)[:mb_h * s, :mb_w * s]))
    return Stim(stim.name + "_1080p", pic.seal(), frame, stim.ref_slots)


def store_of(stim, slots=3):
    """a host frame store with the stimulus picture's reference frames in place"""
    store = oracle_bind.FrameStore(stim.pic.mb_w, stim.pic.mb_h, slots)
    for slot in stim.ref_slots:
        for dst, src in zip(store[slot], stim.frame):
            dst[:] = src
    return store


def expected(oracle, stim, census=None):
    """the decoded picture: prediction and residual by oracle_reconstruct_nodeblock, the loop filter by tests/deblock_checker.py"""
    store = store_of(stim)
    planes = [a.copy() for a in oracle_bind.reconstruct(oracle, store, stim.pic, deblock=False)]
    D.deblock(stim.pic, planes, census)
    return planes


MIN_LINES = 8                # per cell over the stimulus set: a condition on the builder, not a measurement


def check_census(census):
    """every cell of the checker's class list at least MIN_LINES times - none left out, none excused (cells that arithmetic
    excludes are taken off the list by name, with their inequality: deblock_checker.IMPOSSIBLE)"""
    cells = D.all_cells()
    assert len(cells) == len(set(cells)) and len(cells) >= 500
    thin = sorted((census[c], c) for c in cells if census[c] < MIN_LINES)
    assert not thin, "%d of %d cells with fewer than %d lines: %s" % (len(thin), len(cells), MIN_LINES, thin[:12])
    assert not set(census) - set(cells), "the checker counted cells the class list does not know: %s" % sorted(set(census) - set(cells))[:5]
