"""Checker for the loop filter (TEST INFRASTRUCTURE), written from the text of H.264 8.7 - not from oracle/cpu_recon.c
(oracle_deblock_picture / edge / b_motion_strength), not from kernel_deblock.h and not from the reference, which share one reading
of the reference's driver (and shared the comparison of list INDICES in unweighted P pictures until this checker showed it on
lists that hold one frame twice).  Plain Python integers; it calls nothing of the oracle's filter.

`deblock(pic, planes, census)` filters the three planes of an UNFILTERED picture in place (oracle_reconstruct_nodeblock, or one of
the other checkers with its last step left out, supplies them):

* order, 8.7: macroblocks in raster order; per macroblock the luma vertical edges left to right, the luma horizontal edges top to
  bottom, then the same for Cb and for Cr (chroma edges 0 and 2 in units of luma 4x4 blocks; chroma line k takes the strength of
  luma line 2k).  In place: every line reads what earlier edges wrote.
* which edges: the record's `edges` (EDGE_LEFT, EDGE_TOP, EDGE_INNER - filterLeftMbEdgeFlag / filterTopMbEdgeFlag /
  filterInternalEdgesFlag as the slices' disable_deblocking_filter_idc and the picture's borders give them).  What the seam leaves
  undefined raises ValueError: EDGE_LEFT at column 0, EDGE_TOP at row 0, LEFT or TOP without INNER.
* strengths, 8.7.2.1, frame macroblocks: 4 - intra on a macroblock edge; 3 - intra, inner edge; 2 - a 4x4 luma block with
  coefficients on either side (coef_mask bits 0..15); else the motion test BY PICTURE, for P and B alike: different reference
  pictures or a different number of vectors; one vector each, differing by >= 4 quarter-pels in a component; two vectors to two
  different pictures, compared picture by picture; two vectors to the same picture, either pairing.  Pictures are frame-store
  slots (ref_slot[], ref_slot_l1[]); an index at or past its list means entry 0, an inter quadrant with no list at all means
  list 0 entry 0 (include/p264hip.h, ref_idx).
* thresholds, 8.7.2.2: qPp / qPq are the records' qp (I_PCM records carry 0); chroma takes QPC (table 8-15) of each side with
  chroma_qp_offset, then the mean.  indexA / indexB add the descriptor's alpha_c0_offset / beta_offset AS GIVEN: whatever the
  seam carries is what is added.  (The host hands the slice header's slice_alpha_c0_offset_div2 / slice_beta_offset_div2 over
  unshifted, to stay with the reference - SURVEY A-Q3; a caller that wants FilterOffsetA = div2 << 1 passes that.)
* 8.7.2.3 (strength < 4) and 8.7.2.4 (strength 4) per line, Clip1 where the text has it.

The census: per line whose strength is not 0, the classes it falls into (`line_classes` below) - which of the filter's branches it
took - counted per cell = (plane, strength, class, edge direction 'v' / 'h', line parity, 'mb' / 'inner' edge).  `all_cells()` is the
full list a stimulus set has to reach (tests/deblock_stim.py, tests/test_deblock_checker_cpu.py)."""
import collections

import numpy as np

from p264decoder_amd import _native as N

# table 8-16: indexA -> alpha', indexB -> beta'
ALPHA = [0] * 16 + [4, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 17, 20, 22, 25, 28, 32, 36, 40, 45, 50, 56, 63, 71, 80, 90, 101, 113, 127, 144,
                    162, 182, 203, 226, 255, 255]
BETA = [0] * 16 + [2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15, 16, 16, 17, 17,
                   18, 18]
# table 8-17: indexA -> tC0' for bS = 1, 2, 3
TC0 = ([(0, 0, 0)] * 17 + [(0, 0, 1)] * 4 + [(0, 1, 1)] * 2 + [(1, 1, 1)] * 4 + [(1, 1, 2)] * 4 + [(1, 2, 3)] * 2 +
       [(2, 2, 3), (2, 2, 4), (2, 3, 4), (2, 3, 4), (3, 3, 5), (3, 4, 6), (3, 4, 6), (4, 5, 7), (4, 5, 8), (4, 6, 9), (5, 7, 10), (6, 8, 11),
        (6, 8, 13), (7, 10, 14), (8, 11, 16), (9, 12, 18), (10, 13, 20), (11, 15, 23), (13, 17, 25)])
assert len(ALPHA) == len(BETA) == len(TC0) == 52
# table 8-15: qPI -> QPC
CHROMA_QP = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
assert len(CHROMA_QP) == 52
# 4x4 luma blocks in decoding order -> position in units of blocks (6.4.3, figure 6-10)
BLK_X = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
BLK_Y = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]
BLK_AT = {(BLK_X[i], BLK_Y[i]): i for i in range(16)}


def clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def thresholds(qp_av, off_a, off_b):
    """8.7.2.2: (indexA, alpha, beta) of an edge with the mean QP qp_av (8-bit samples: alpha = alpha', beta = beta')"""
    ia, ib = clip3(0, 51, qp_av + off_a), clip3(0, 51, qp_av + off_b)
    return ia, ALPHA[ia], BETA[ib]


def chroma_qp_av(qp_p, qp_q, cqo):
    """8.7.2.2, chroma: QPC of each side, then the mean"""
    return (CHROMA_QP[clip3(0, 51, qp_p + cqo)] + CHROMA_QP[clip3(0, 51, qp_q + cqo)] + 1) >> 1


# ---- classes ------------------------------------------------------------------------------------------------------------------
def line_classes(chroma, bs):
    """every class a line of that plane kind and strength can fall into (a line falls into several: one per group)"""
    out = ["off/alpha=0", "off/alpha>0"]
    if bs < 4:
        out += ["delta %s/%s" % (a, b) for a in ("saturates", "inside") for b in ("tc0=0", "tc0>0")]
        out += ["clipped at 0", "clipped at 255"]
        if not chroma:
            out += ["ap%d aq%d" % (a, b) for a in (0, 1) for b in (0, 1)]
            out += ["p1 saturates", "p1 inside", "q1 saturates", "q1 inside"]
    elif chroma:
        out += ["strong"]
    else:
        out += ["small%d ap%d aq%d" % (s, a, b) for s in (0, 1) for a in (0, 1) for b in (0, 1)]
    return out


# Classes that arithmetic excludes, by name with the inequality (none is excused silently; tests/test_deblock_checker_cpu.py asserts
# that every other cell occurs):
#   (none so far: every class above has a line that reaches it - see tests/deblock_stim.py, `propose`)
IMPOSSIBLE = set()


def all_cells():
    """(plane, strength, class, direction, parity, where): strengths 1 and 2 occur on macroblock edges and inner edges, 3 on inner
    edges only, 4 on macroblock edges only (8.7.2.1, frame macroblocks)"""
    cells = []
    for plane in "yc":
        for bs in (1, 2, 3, 4):
            for where in (("mb", "inner") if bs < 3 else ("inner",) if bs == 3 else ("mb",)):
                for cl in line_classes(plane == "c", bs):
                    if (plane, bs, cl) in IMPOSSIBLE:
                        continue
                    for d in "vh":
                        for parity in (0, 1):
                            cells.append((plane, bs, cl, d, parity, where))
    return cells


# ---- 8.7.2.2 - 8.7.2.4: one line ----------------------------------------------------------------------------------------------
def filter_line(s, chroma, bs, index_a, alpha, beta, hits=None):
    """s: the samples across the edge, luma p3 p2 p1 p0 q0 q1 q2 q3, chroma p1 p0 q0 q1.  Returns the filtered samples (a new
    list, or s itself when nothing applies); hits (a list) receives the names of the classes the line fell into."""
    if bs == 0:
        return s
    hit = hits.append if hits is not None else (lambda _: None)
    if chroma:
        p1, p0, q0, q1 = s
    else:
        p3, p2, p1, p0, q0, q1, q2, q3 = s
    # filterSamplesFlag (8-468)
    if not (abs(p0 - q0) < alpha and abs(p1 - p0) < beta and abs(q1 - q0) < beta):
        hit("off/alpha=0" if alpha == 0 else "off/alpha>0")
        return s
    if bs < 4:                                                  # 8.7.2.3
        tc0 = TC0[index_a][bs - 1]
        if chroma:
            tc = tc0 + 1
        else:
            ap, aq = abs(p2 - p0), abs(q2 - q0)
            tc = tc0 + (1 if ap < beta else 0) + (1 if aq < beta else 0)
        raw = (((q0 - p0) << 2) + (p1 - q1) + 4) >> 3
        delta = clip3(-tc, tc, raw)
        hit("delta %s/%s" % ("saturates" if delta != raw else "inside", "tc0=0" if tc0 == 0 else "tc0>0"))
        P0, Q0 = clip3(0, 255, p0 + delta), clip3(0, 255, q0 - delta)        # Clip1
        if p0 + delta < 0 or q0 - delta < 0:
            hit("clipped at 0")
        if p0 + delta > 255 or q0 - delta > 255:
            hit("clipped at 255")
        if chroma:
            return [p1, P0, Q0, q1]
        hit("ap%d aq%d" % (ap < beta, aq < beta))
        P1, Q1 = p1, q1
        if ap < beta:
            r = (p2 + ((p0 + q0 + 1) >> 1) - (p1 << 1)) >> 1
            c = clip3(-tc0, tc0, r)
            hit("p1 saturates" if c != r else "p1 inside")
            P1 = p1 + c
        if aq < beta:
            r = (q2 + ((p0 + q0 + 1) >> 1) - (q1 << 1)) >> 1
            c = clip3(-tc0, tc0, r)
            hit("q1 saturates" if c != r else "q1 inside")
            Q1 = q1 + c
        return [p3, p2, P1, P0, Q0, Q1, q2, q3]
    # 8.7.2.4
    if chroma:
        hit("strong")
        return [p1, (2 * p1 + p0 + q1 + 2) >> 2, (2 * q1 + q0 + p1 + 2) >> 2, q1]
    ap, aq = abs(p2 - p0), abs(q2 - q0)
    small = abs(p0 - q0) < ((alpha >> 2) + 2)
    hit("small%d ap%d aq%d" % (small, ap < beta, aq < beta))
    if ap < beta and small:
        P0 = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3
        P1 = (p2 + p1 + p0 + q0 + 2) >> 2
        P2 = (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3
    else:
        P0, P1, P2 = (2 * p1 + p0 + q1 + 2) >> 2, p1, p2
    if aq < beta and small:
        Q0 = (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3
        Q1 = (p0 + q0 + q1 + q2 + 2) >> 2
        Q2 = (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3
    else:
        Q0, Q1, Q2 = (2 * q1 + q0 + p1 + 2) >> 2, q1, q2
    return [p3, P2, P1, P0, Q0, Q1, Q2, q3]


# ---- 8.7.2.1: strengths -------------------------------------------------------------------------------------------------------
def _uses(pic, m, x, y):
    """the predictions of the 4x4 block (x, y) of inter macroblock m: [(picture, mvx, mvy)], one per list it uses"""
    d = pic.desc
    q = m * 4 + (y >> 1) * 2 + (x >> 1)
    r0 = int(pic.ref_idx[q])
    r1 = int(pic.ref_idx_l1[q]) if d.slice_type == N.SLICE_B else -1
    if r0 < 0 and r1 < 0:
        r0 = 0                                                  # no list at all: list 0, entry 0
    i = (m * 16 + y * 4 + x) * 2
    out = []
    if r0 >= 0:
        out.append((int(d.ref_slot[r0 if r0 < d.n_ref else 0]), int(pic.mv[i]), int(pic.mv[i + 1])))
    if r1 >= 0:
        out.append((int(d.ref_slot_l1[r1 if r1 < d.n_ref_l1 else 0]), int(pic.mv_l1[i]), int(pic.mv_l1[i + 1])))
    return out


def _far(a, b):
    return abs(a[1] - b[1]) >= 4 or abs(a[2] - b[2]) >= 4


def motion_strength(pic, m, x, y, n, xn, yn):
    """the last rules of 8.7.2.1 for two inter blocks without coefficients: 1 or 0"""
    P, Q = _uses(pic, n, xn, yn), _uses(pic, m, x, y)
    if len(P) != len(Q) or sorted(u[0] for u in P) != sorted(u[0] for u in Q):
        return 1                                                # different reference pictures or a different number of vectors
    if len(P) == 1:
        return int(_far(P[0], Q[0]))
    if P[0][0] != P[1][0]:                                      # two different pictures: the vectors of the same picture
        by_pic = {u[0]: u for u in Q}
        return int(any(_far(u, by_pic[u[0]]) for u in P))
    straight = not _far(P[0], Q[0]) and not _far(P[1], Q[1])   # both vectors to one picture: either pairing will do
    crossed = not _far(P[0], Q[1]) and not _far(P[1], Q[0])
    return int(not (straight or crossed))


def edge_strengths(pic, m, d, e):
    """the four strengths (one per 4-line segment) of edge e (0 = the macroblock edge) in direction d (0 vertical edges) of
    macroblock m, and the neighbouring macroblock p lies in"""
    rec = pic.mb_records()
    n = m if e else (m - 1 if d == 0 else m - pic.mb_w)
    if rec["mb_type"][m] <= N.MB_IPCM or rec["mb_type"][n] <= N.MB_IPCM:
        return [4 if e == 0 else 3] * 4, n
    out = []
    cm, cn = int(rec["coef_mask"][m]), int(rec["coef_mask"][n])
    for i in range(4):
        x, y = (e, i) if d == 0 else (i, e)
        xn, yn = ((x - 1) & 3, y) if d == 0 else (x, (y - 1) & 3)
        if (cm >> BLK_AT[(x, y)]) & 1 or (cn >> BLK_AT[(xn, yn)]) & 1:
            out.append(2)
        else:
            out.append(motion_strength(pic, m, x, y, n, xn, yn))
    return out, n


# ---- 8.7: the picture ---------------------------------------------------------------------------------------------------------
def check_edges(pic):
    """ValueError for everything about `edges` that the seam leaves undefined"""
    rec = pic.mb_records()
    for m in range(pic.n_mb):
        e = int(rec["edges"][m])
        if e & N.EDGE_LEFT and m % pic.mb_w == 0:
            raise ValueError("macroblock %d: EDGE_LEFT at column 0" % m)
        if e & N.EDGE_TOP and m < pic.mb_w:
            raise ValueError("macroblock %d: EDGE_TOP at row 0" % m)
        if e & (N.EDGE_LEFT | N.EDGE_TOP) and not e & N.EDGE_INNER:
            raise ValueError("macroblock %d: a macroblock edge is filtered and the inner edges are not (edges = %d)" % (m, e))


def deblock(pic, planes, census=None):
    """planes: [y, u, v] of the unfiltered picture, uint8, filtered in place.  Returns the census (a Counter of cells)."""
    census = collections.Counter() if census is None else census
    check_edges(pic)
    d = pic.desc
    rec = pic.mb_records()
    off_a, off_b, cqo = int(d.alpha_c0_offset), int(d.beta_offset), int(d.chroma_qp_offset)
    work = [p.astype(np.int64).tolist() for p in planes]        # lists of rows of ints: much faster to walk than arrays
    hits = []
    for m in range(pic.n_mb):
        flags = int(rec["edges"][m])
        if not flags:
            continue
        mbx, mby = m % pic.mb_w, m // pic.mb_w
        strengths = {}
        for dr in (0, 1):
            for e in range(4):
                if e == 0 and not flags & (N.EDGE_LEFT if dr == 0 else N.EDGE_TOP):
                    continue
                strengths[(dr, e)] = edge_strengths(pic, m, dr, e)
        qp = int(rec["qp"][m])
        for pl in range(3):
            chroma = pl > 0
            P = work[pl]
            size, half, step = (8, 2, 2) if chroma else (16, 4, 1)          # macroblock size, samples per side, edge step in 4x4 units
            x0, y0 = mbx * size, mby * size
            for dr in (0, 1):
                for e in range(0, 4, step):
                    if (dr, e) not in strengths:
                        continue
                    bs4, n = strengths[(dr, e)]
                    if not any(bs4):
                        continue
                    qn = int(rec["qp"][n])
                    qp_av = chroma_qp_av(qn, qp, cqo) if chroma else (qn + qp + 1) >> 1
                    ia, alpha, beta = thresholds(qp_av, off_a, off_b)
                    at = (e * 4) >> (1 if chroma else 0)                    # the edge's offset inside the macroblock, in samples
                    where = "inner" if e else "mb"
                    for k in range(size):
                        bs = bs4[(k * 4) // size]
                        if bs == 0:
                            continue
                        if dr == 0:
                            row = P[y0 + k]
                            a = x0 + at - half
                            s = row[a:a + 2 * half]
                        else:
                            a = y0 + at - half
                            s = [P[a + j][x0 + k] for j in range(2 * half)]
                        del hits[:]
                        o = filter_line(s, chroma, bs, ia, alpha, beta, hits)
                        for cl in hits:
                            census[("c" if chroma else "y", bs, cl, "vh"[dr], k & 1, where)] += 1
                        if o is not s:
                            if dr == 0:
                                row[a:a + 2 * half] = o
                            else:
                                for j in range(2 * half):
                                    P[a + j][x0 + k] = o[j]
    for p, w in zip(planes, work):
        p[:] = np.array(w, np.int64).astype(np.uint8)
    return census
