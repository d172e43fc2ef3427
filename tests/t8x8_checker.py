"""Checker for inter macroblocks coded with the 8x8 transform (TEST INFRASTRUCTURE), written from the text of H.264 - 8.5.6 (the
inverse 8x8 zig-zag scan of frame macroblocks), 8.5.9 / 8.5.13 (scaling with Flat_8x8_16: LevelScale8x8 = 16 * normAdjust8x8, both
branches qP >= 36 / qP < 36; the transform, every row then every column, (m + 32) >> 6), 8.5.14 (Clip1) and 8.7 (luma edges 1 and 3
of such a macroblock are no transform edges: not filtered) - not from kernel_t8x8.h.  Python integers; the oracle knows nothing of
the flag and is not involved.

A record with N.MB_T8X8 in intra_modes (include/p264hip.h): bits 0-15 of coef_mask in nibbles, nibble k = 0xF where the luma 8x8
block k (quadrants in raster order) is coded; a coded block is FOUR consecutive sixteen-level entries of coefs[], its 64 levels in
scan order, at the place the 4x4 rule gives (block_at of the nibble's lowest bit).  Chroma is as on every record.

Range: 8.5.13 bounds, for a conformant stream, the scaled values and every intermediate of both stages to -2^15 .. 2^15 - 1;
`block8x8` records them in a residual_checker.Range and `luma8x8_of` refuses (OutOfRange) a macroblock with a value outside.

`SpecRecon` is spec_recon.SpecRecon with the luma of flagged macroblocks taken from here and a loop filter that skips their luma
edges 1 and 3; it counts the lines where filtering a skipped edge would have changed a sample (`tells`: what a filter that ignores
the flag gets wrong)."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker, residual_checker, spec_recon
from tests.deblock_checker import check_edges, chroma_qp_av, edge_strengths, filter_line, thresholds
from tests.residual_checker import OutOfRange, Range
from tests.slice_filter_checker import offsets_of

# 8.5.6, 8x8 frame scan: scan index -> x + 8 * y
SCAN8 = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
assert sorted(SCAN8) == list(range(64))
# normAdjust8x8: v[m][class]; the class of position (i, j) by (i & 3) * 4 + (j & 3)
V8 = [(20, 18, 32, 19, 25, 24), (22, 19, 35, 21, 28, 26), (26, 23, 42, 24, 33, 31), (28, 25, 45, 26, 35, 33), (32, 28, 51, 30, 40, 38), (36, 32, 58, 34, 46, 43)]
CLASS8 = [0, 3, 4, 3, 3, 1, 5, 1, 4, 5, 2, 5, 3, 1, 5, 1]


def flagged(r):
    return bool(int(r["intra_modes"]) & N.MB_T8X8)


def level_scale8(m, i, j):
    return 16 * V8[m][CLASS8[(i & 3) * 4 + (j & 3)]]


def unscan8(levels):
    """64 levels in scan order -> c[i][j], i the row"""
    c = [[0] * 8 for _ in range(8)]
    for k in range(64):
        c[SCAN8[k] >> 3][SCAN8[k] & 7] = int(levels[k])
    return c


def scale8x8(c, qp, rng):
    s = qp // 6
    if qp >= 36:
        d = [[(c[i][j] * level_scale8(qp % 6, i, j)) << (s - 6) for j in range(8)] for i in range(8)]
    else:
        d = [[(c[i][j] * level_scale8(qp % 6, i, j) + (1 << (5 - s))) >> (6 - s) for j in range(8)] for i in range(8)]
    rng.see("d", [x for r in d for x in r])
    return d


def stage(d, rng=None, name=""):
    """the one-dimensional transform of 8.5.13 on d[0 .. 7]"""
    a = [d[0] + d[4], -d[3] + d[5] - d[7] - (d[7] >> 1), (d[2] >> 1) - d[6], d[1] + d[7] - d[3] - (d[3] >> 1),
         d[0] - d[4], -d[1] + d[7] + d[5] + (d[5] >> 1), d[2] + (d[6] >> 1), d[3] + d[5] + d[1] + (d[1] >> 1)]
    b = [a[0] + a[6], a[1] + (a[7] >> 2), a[4] + a[2], a[3] + (a[5] >> 2), a[4] - a[2], (a[3] >> 2) - a[5], a[0] - a[6], a[7] - (a[1] >> 2)]
    out = [b[0] + b[7], b[2] + b[5], b[4] + b[3], b[6] + b[1], b[6] - b[1], b[4] - b[3], b[2] - b[5], b[0] - b[7]]
    if rng is not None:
        rng.see(name + " a", a)
        rng.see(name + " b", b)
        rng.see(name + " out", out)
    return out


def transform8x8(d, rng):
    """8.5.13: every row first, then every column; r = (m + 32) >> 6"""
    g = [stage(d[i], rng, "row") for i in range(8)]
    cols = [stage([g[i][j] for i in range(8)], rng, "column") for j in range(8)]
    return [[(cols[j][i] + 32) >> 6 for j in range(8)] for i in range(8)]


def block8x8(levels, qp, rng):
    return transform8x8(scale8x8(unscan8(levels), qp, rng), rng)


def levels8_of(pic, r, k):
    """the 64 levels of the coded luma 8x8 block k of the flagged record r"""
    at = residual_checker.block_at(r, 1 << (4 * k)) * 16
    return [int(v) for v in pic.coefs[at:at + 64]]


def check_record(r):
    mask = int(r["coef_mask"])
    assert int(r["mb_type"]) > N.MB_IPCM, "MB_T8X8 on an intra record"
    assert all((mask >> (4 * k)) & 15 in (0, 15) for k in range(4)), "luma nibbles of %#x" % mask


def luma8x8_of(pic, m, refuse=True):
    """({quadrant k: r[8][8]} of the coded 8x8 blocks of the flagged macroblock m, the Range of everything bounded on the way)"""
    r = pic.mb_records()[m]
    check_record(r)
    out, rng = {}, Range()
    for k in range(4):
        if (int(r["coef_mask"]) >> (4 * k)) & 1:
            out[k] = block8x8(levels8_of(pic, r, k), int(r["qp"]), rng)
    if refuse and not rng.ok:
        raise OutOfRange("macroblock %d (8x8 transform): %s outside -2^15 .. 2^15 - 1: H.264 defines no result" % (m, sorted(set(rng.bad))))
    return out, rng


def chroma_residual_of(pic, m):
    """{(plane, x, y): r[4][4]} of the chroma of flagged macroblock m, by residual_checker on a one-macroblock picture that holds
    the record's chroma entries alone (chroma DC, then the AC blocks: the luma entries between them taken out)"""
    r = pic.mb_records()[m]
    mask, at = int(r["coef_mask"]), int(r["coef_index"])
    n_luma = bin(mask & 0xffff).count("1")
    has_dc = 1 if mask & N.COEF_CHROMA_DC else 0
    n_ac = bin(mask & 0xff0000).count("1")
    lv = np.concatenate([np.asarray(pic.coefs[at * 16:(at + has_dc) * 16]), np.asarray(pic.coefs[(at + has_dc + n_luma) * 16:(at + has_dc + n_luma + n_ac) * 16]),
                         np.zeros(16, np.int16)]).astype(np.int16)

    class One:
        desc = pic.desc
        coefs = lv

        @staticmethod
        def mb_records():
            rr = np.array([r])
            rr["coef_mask"][0] = mask & ~0xffff
            rr["coef_index"][0] = 0
            return rr
    res, _, _ = residual_checker.residual_of(One, 0)
    return {k: v for k, v in res.items() if k[0]}


def add_residual(pic, m, F):
    """8.5.14 for the flagged macroblock m on the planes F = [y, u, v], which hold its prediction"""
    d = pic.desc
    x0, y0 = (m % d.mb_w) * 16, (m // d.mb_w) * 16
    for k, r in luma8x8_of(pic, m)[0].items():
        bx, by = x0 + (k & 1) * 8, y0 + (k >> 1) * 8
        for i in range(8):
            for j in range(8):
                F[0][by + i, bx + j] = min(max(int(F[0][by + i, bx + j]) + r[i][j], 0), 255)
    for (plane, x, y), r in chroma_residual_of(pic, m).items():
        residual_checker.construct(F[plane], (x0 >> 1) + x, (y0 >> 1) + y, r)


def deblock(pic, planes, tells=None):
    """8.7 on the unfiltered planes [y, u, v], in place: tests/slice_filter_checker.py's walk (the offsets of the macroblock that
    holds q0) without the luma edges 1 and 3 of flagged macroblocks.  tells: a Counter - per direction 'v' / 'h', the lines of the
    skipped edges that the filter would have changed.  Returns it."""
    tells = collections.Counter() if tells is None else tells
    check_edges(pic)
    d = pic.desc
    rec = pic.mb_records()
    cqo = int(d.chroma_qp_offset)
    work = [p.astype(np.int64).tolist() for p in planes]
    for m in range(pic.n_mb):
        flags = int(rec["edges"][m])
        if not flags:
            continue
        mbx, mby = m % pic.mb_w, m // pic.mb_w
        off_a, off_b = offsets_of(pic, m)
        t8 = flagged(rec[m])
        qp = int(rec["qp"][m])
        for pl in range(3):
            chroma = pl > 0
            P = work[pl]
            size, half, step = (8, 2, 2) if chroma else (16, 4, 1)
            x0, y0 = mbx * size, mby * size
            for dr in (0, 1):
                for e in range(0, 4, step):
                    if e == 0 and not flags & (N.EDGE_LEFT if dr == 0 else N.EDGE_TOP):
                        continue
                    skipped = t8 and not chroma and e in (1, 3)
                    bs4, n = edge_strengths(pic, m, dr, e)
                    if not any(bs4):
                        continue
                    qn = int(rec["qp"][n])
                    qp_av = chroma_qp_av(qn, qp, cqo) if chroma else (qn + qp + 1) >> 1
                    ia, alpha, beta = thresholds(qp_av, off_a, off_b)
                    at = (e * 4) >> (1 if chroma else 0)
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
                        o = filter_line(s, chroma, bs, ia, alpha, beta)
                        if o is s or list(o) == list(s):
                            continue
                        if skipped:
                            tells["vh"[dr]] += 1
                        elif dr == 0:
                            row[a:a + 2 * half] = o
                        else:
                            for j in range(2 * half):
                                P[a + j][x0 + k] = o[j]
    for p, w in zip(planes, work):
        p[:] = np.array(w, np.int64).astype(np.uint8)
    return tells


class SpecRecon(spec_recon.SpecRecon):
    """spec_recon.SpecRecon for pictures whose inter records may carry N.MB_T8X8"""

    def __init__(self, mb_w, mb_h, slots):
        super().__init__(mb_w, mb_h, slots)
        self.tells = collections.Counter()

    def _inter(self, pic):
        F = inter_checker.predict(pic, self.store, self.census)
        rec = pic.mb_records()
        for m in np.flatnonzero(rec["mb_type"] > N.MB_IPCM):
            if flagged(rec[m]):
                add_residual(pic, int(m), F)
            else:
                residual_checker.add_residual(pic, int(m), F)

    def reconstruct(self, pic):
        F = self.nodeblock(pic)
        if pic.desc.deblock:
            deblock(pic, F, self.tells)
        return F
