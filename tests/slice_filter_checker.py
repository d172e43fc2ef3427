"""Checker for the loop filter of pictures whose macroblocks carry their own filter offsets (TEST INFRASTRUCTURE): the picture
loop of tests/deblock_checker.py, typed from H.264 8.7 as that module is, with ONE difference - filterOffsetA / filterOffsetB of
an edge are those of the macroblock whose left, top or inner edge is being filtered (8.7.2.2: the slice that holds q0), i.e. the
descriptor's alpha_c0_offset / beta_offset plus the two signed deltas in the record's `flags` (include/p264hip.h: bits 0-7 alpha,
bits 8-15 beta, added as given).  Both QPs of the edge still count.  Everything else - the line filters, the tables, the
strengths, the checks on `edges`, the census - is deblock_checker's, imported unchanged; the oracle's filter, which knows one
offset pair per picture, is not involved.

With every `flags` zero this is deblock_checker.deblock byte for byte (tests/test_slice_filter_cpu.py).

Besides the census the walk counts, per line that the filter works on (strength not 0 and filterSamplesFlag set):

* `seams`: lines of a LEFT or TOP macroblock edge whose two macroblocks carry different offsets, per cell
  (edge 'left' / 'top', plane 'y' / 'c', strength '<4' / '4');
* `inner`: lines of the inner edges of a macroblock whose offsets differ from the picture's, per cell
  (direction 'v' / 'h', plane 'y' / 'c', strength '<3' / '3').  Strength 4 does not exist on an inner edge of a frame
  macroblock (8.7.2.1: 4 needs a macroblock edge), so the strongest an inner edge takes, 3, stands in its place;
* `tells` (same cells as both, prefixed 'seam' / 'inner'): those of the lines above whose result differs from what the OTHER
  offsets would have given - the p macroblock's on a macroblock edge, the picture's on an inner edge.  These are the lines a
  filter that takes the wrong macroblock's offsets, or ignores the deltas, gets wrong.
"""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests.deblock_checker import check_edges, chroma_qp_av, edge_strengths, filter_line, thresholds


def flags_of(alpha_delta, beta_delta):
    """the record's `flags` for two signed deltas (int8 each)"""
    assert -128 <= alpha_delta <= 127 and -128 <= beta_delta <= 127
    return (alpha_delta & 255) | ((beta_delta & 255) << 8)


def deltas_of(flags):
    """(alpha delta, beta delta) of a record's `flags`"""
    a, b = flags & 255, (flags >> 8) & 255
    return a - 256 if a > 127 else a, b - 256 if b > 127 else b


def offsets_of(pic, m):
    """filterOffsetA / filterOffsetB of macroblock m, in the seam's units"""
    a, b = deltas_of(int(pic.mb_records()["flags"][m]))
    return int(pic.desc.alpha_c0_offset) + a, int(pic.desc.beta_offset) + b


SEAM_CELLS = [(e, p, s) for e in ("left", "top") for p in "yc" for s in ("<4", "4")]
INNER_CELLS = [(d, p, s) for d in "vh" for p in "yc" for s in ("<3", "3")]


class Counts:
    """what a walk saw besides the census (see the module's text)"""

    def __init__(self):
        self.census = collections.Counter()
        self.seams = collections.Counter()
        self.inner = collections.Counter()
        self.tells = collections.Counter()

    def missing(self):
        """the cells of the coverage tables no line fell into"""
        out = [("seam",) + c for c in SEAM_CELLS if not self.seams[c]] + [("inner",) + c for c in INNER_CELLS if not self.inner[c]]
        out += [("tell", k) + c for k, cells in (("seam", SEAM_CELLS), ("inner", INNER_CELLS)) for c in cells if not self.tells[(k,) + c]]
        return out


def deblock(pic, planes, counts=None):
    """planes: [y, u, v] of the unfiltered picture, uint8, filtered in place.  Returns the Counts."""
    counts = Counts() if counts is None else counts
    census = counts.census
    check_edges(pic)
    d = pic.desc
    rec = pic.mb_records()
    cqo = int(d.chroma_qp_offset)
    pic_off = (int(d.alpha_c0_offset), int(d.beta_offset))
    work = [p.astype(np.int64).tolist() for p in planes]
    hits = []
    for m in range(pic.n_mb):
        flags = int(rec["edges"][m])
        if not flags:
            continue
        mbx, mby = m % pic.mb_w, m // pic.mb_w
        off_a, off_b = offsets_of(pic, m)                       # the macroblock that holds q0, for every one of its edges
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
            size, half, step = (8, 2, 2) if chroma else (16, 4, 1)
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
                    other = offsets_of(pic, n) if e == 0 else pic_off            # what a wrong reading would take
                    differs = other != (off_a, off_b)
                    if differs:
                        ia_o, alpha_o, beta_o = thresholds(qp_av, other[0], other[1])
                    at = (e * 4) >> (1 if chroma else 0)
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
                        if differs:
                            plane = "c" if chroma else "y"
                            if e == 0:
                                kind, cell = "seam", (("left", "top")[dr], plane, "4" if bs == 4 else "<4")
                            else:
                                kind, cell = "inner", ("vh"[dr], plane, "3" if bs == 3 else "<3")
                            if o is not s:
                                (counts.seams if e == 0 else counts.inner)[cell] += 1
                            if list(filter_line(s, chroma, bs, ia_o, alpha_o, beta_o)) != list(o) and o is not s:
                                counts.tells[(kind,) + cell] += 1
                        if o is not s:
                            if dr == 0:
                                row[a:a + 2 * half] = o
                            else:
                                for j in range(2 * half):
                                    P[a + j][x0 + k] = o[j]
    for p, w in zip(planes, work):
        p[:] = np.array(w, np.int64).astype(np.uint8)
    return counts
