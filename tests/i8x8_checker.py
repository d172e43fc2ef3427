"""Checker for Intra 8x8 macroblocks (TEST INFRASTRUCTURE), written from the text of H.264 8.3.2 - the derivation of the 25
reference samples p[-1, -1], p[0..15, -1], p[-1, 0..7] with the availability of 8.3.2.2 (6.4.11.2: neighbouring 8x8 blocks), the
reference sample filter of 8.3.2.2.1 with its end and corner cases, and the nine predictors of 8.3.2.2.2 - 8.3.2.2.10 - not from
kernel_intra.h and not from oracle/, which knows nothing of the flag.  Python integers.

A record with N.MB_I8X8 in intra_modes (include/p264hip.h) is an I4x4 record whose luma is laid out as tests/t8x8_checker.py reads
it (whole nibbles, four entries per coded 8x8 block); i4modes[4k] is Intra8x8PredMode of 8x8 block k.  The residual is that
module's block8x8 (8.5.6, 8.5.9, 8.5.13).

A sample that is not available is None: a predictor that reads one raises ValueError - never a substitute.

`Census` records what the predicted blocks exercised: (mode, block index, (left, top, top-left, top-right)), the branches of the
filter that ran, the DC cases.  `SpecRecon` is t8x8_checker.SpecRecon with Intra 8x8 macroblocks and a loop filter that skips luma
edges 1 and 3 for either flag."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import intra_checker, residual_checker, spec_recon
from tests import t8x8_checker as T8
from tests.residual_checker import OutOfRange, Range

MODE8_NAMES = intra_checker.MODE4_NAMES


def flagged(r):
    return bool(int(r["intra_modes"]) & N.MB_I8X8)


def block_availability(k, L, T, TR, TL):
    """(left, top, top-left, top-right) of luma 8x8 block k (quadrants in raster order) from the macroblock's four flags (6.4.11.2:
    block 3's top-right neighbour lies in a macroblock that is decoded later - never available)"""
    return ((bool(L), bool(T), bool(TL), bool(T)), (True, bool(T), bool(T), bool(TR)), (bool(L), True, bool(L), True), (True, True, True, False))[k]


def needs(mode):
    """(left, top, top-left) a mode reads (8.3.2.2.2 - 10: what must be 'available for Intra_8x8 prediction')"""
    return {0: (0, 1, 0), 1: (1, 0, 0), 2: (0, 0, 0), 3: (0, 1, 0), 4: (1, 1, 1), 5: (1, 1, 1), 6: (1, 1, 1), 7: (0, 1, 0), 8: (1, 0, 0)}[mode]


def legal_modes(left, top, topleft):
    return [m for m in range(9) if all(have or not need for need, have in zip(needs(m), (left, top, topleft)))]


class Census:
    def __init__(self):
        self.blocks = collections.Counter()     # (mode, block, (left, top, topleft, topright))
        self.filter = collections.Counter()     # names of the filter's cases
        self.dc = collections.Counter()         # "both" / "left" / "top" / "none"


def reference_samples(left, top, topright, corner):
    """8.3.2.2: left = p[-1, 0..7], top = p[0..7, -1], topright = p[8..15, -1] (each a sequence or None), corner = p[-1, -1] or None.
    Returns (left, top16, corner): where the top is available and the top-right is not, p[7, -1] stands in for p[8..15, -1]."""
    top16 = None
    if top is not None:
        t = [int(v) for v in top]
        top16 = t + ([int(v) for v in topright] if topright is not None else [t[7]] * 8)
    return (None if left is None else [int(v) for v in left]), top16, (None if corner is None else int(corner))


def filter_samples(left, top16, corner, census=None):
    """8.3.2.2.1: p -> p'.  Same shapes as reference_samples returns."""
    see = (lambda name: census.filter.update([name])) if census is not None else (lambda name: None)
    ft = fl = fc = None
    if top16 is not None:
        p = top16
        ft = [0] * 16
        if corner is not None:
            ft[0] = (corner + 2 * p[0] + p[1] + 2) >> 2
            see("top[0] with corner")
        else:
            ft[0] = (3 * p[0] + p[1] + 2) >> 2
            see("top[0] without corner")
        for x in range(1, 15):
            ft[x] = (p[x - 1] + 2 * p[x] + p[x + 1] + 2) >> 2
        ft[15] = (p[14] + 3 * p[15] + 2) >> 2
        see("top[15]")
    if corner is not None:
        if top16 is None or left is None:
            if top16 is not None:
                fc = (3 * corner + top16[0] + 2) >> 2
                see("corner with top only")
            elif left is not None:
                fc = (3 * corner + left[0] + 2) >> 2
                see("corner with left only")
            else:
                fc = corner
                see("corner alone")
        else:
            fc = (top16[0] + 2 * corner + left[0] + 2) >> 2
            see("corner with both")
    if left is not None:
        p = left
        fl = [0] * 8
        if corner is not None:
            fl[0] = (corner + 2 * p[0] + p[1] + 2) >> 2
            see("left[0] with corner")
        else:
            fl[0] = (3 * p[0] + p[1] + 2) >> 2
            see("left[0] without corner")
        for y in range(1, 7):
            fl[y] = (p[y - 1] + 2 * p[y] + p[y + 1] + 2) >> 2
        fl[7] = (p[6] + 3 * p[7] + 2) >> 2
        see("left[7]")
    return fl, ft, fc


def pred8x8(mode, left, top16, corner, census=None):
    """Intra 8x8 prediction from the FILTERED samples p' (8.3.2.2.2 - 8.3.2.2.10): int[8][8] indexed [y][x]"""
    if not 0 <= mode <= 8:
        raise ValueError("Intra8x8 mode %d" % mode)
    p = intra_checker._Edge(left, top16, corner, "Intra8x8 %s" % MODE8_NAMES[mode])
    o = np.zeros((8, 8), np.int64)
    if mode == 2:
        if left is not None and top16 is not None:
            v, case = (sum(top16[:8]) + sum(left) + 8) >> 4, "both"
        elif left is not None:
            v, case = (sum(left) + 4) >> 3, "left"
        elif top16 is not None:
            v, case = (sum(top16[:8]) + 4) >> 3, "top"
        else:
            v, case = 128, "none"
        if census is not None:
            census.dc[case] += 1
        o[:] = v
        return o
    for y in range(8):
        for x in range(8):
            if mode == 0:
                v = p(x, -1)
            elif mode == 1:
                v = p(-1, y)
            elif mode == 3:
                v = (p(14, -1) + 3 * p(15, -1) + 2) >> 2 if x == 7 and y == 7 else (p(x + y, -1) + 2 * p(x + y + 1, -1) + p(x + y + 2, -1) + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
            elif mode == 5:
                z, k = 2 * x - y, x - (y >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (p(k - 1, -1) + p(k, -1) + 1) >> 1
                elif z >= 0:
                    v = (p(k - 2, -1) + 2 * p(k - 1, -1) + p(k, -1) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(-1, y - 2 * x - 1) + 2 * p(-1, y - 2 * x - 2) + p(-1, y - 2 * x - 3) + 2) >> 2
            elif mode == 6:
                z, k = 2 * y - x, y - (x >> 1)
                if z >= 0 and z % 2 == 0:
                    v = (p(-1, k - 1) + p(-1, k) + 1) >> 1
                elif z >= 0:
                    v = (p(-1, k - 2) + 2 * p(-1, k - 1) + p(-1, k) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(x - 2 * y - 1, -1) + 2 * p(x - 2 * y - 2, -1) + p(x - 2 * y - 3, -1) + 2) >> 2
            elif mode == 7:
                k = x + (y >> 1)
                v = (p(k, -1) + p(k + 1, -1) + 1) >> 1 if y % 2 == 0 else (p(k, -1) + 2 * p(k + 1, -1) + p(k + 2, -1) + 2) >> 2
            else:
                z, k = x + 2 * y, y + (x >> 1)
                if z > 13:
                    v = p(-1, 7)
                elif z == 13:
                    v = (p(-1, 6) + 3 * p(-1, 7) + 2) >> 2
                elif z % 2 == 0:
                    v = (p(-1, k) + p(-1, k + 1) + 1) >> 1
                else:
                    v = (p(-1, k) + 2 * p(-1, k + 1) + p(-1, k + 2) + 2) >> 2
            o[y, x] = v
    return o


def predict_block(Y, x, y, mode, avail, census=None, k=None):
    """the prediction of the 8x8 block at (x, y) of plane Y with avail = (left, top, top-left, top-right)"""
    bl, bt, bc, btr = avail
    left = Y[y:y + 8, x - 1].tolist() if bl else None
    top = Y[y - 1, x:x + 8].tolist() if bt else None
    tr = Y[y - 1, x + 8:x + 16].tolist() if btr else None
    corner = int(Y[y - 1, x - 1]) if bc else None
    if census is not None:
        census.blocks[(mode, k, tuple(avail))] += 1
    fl, ft, fc = filter_samples(*reference_samples(left, top, tr, corner), census=census)
    return pred8x8(mode, fl, ft, fc, census)


def check_record(r):
    mask, modes = int(r["coef_mask"]), int(r["intra_modes"])
    assert int(r["mb_type"]) == N.MB_I4x4, "MB_I8X8 on a record that is not I4x4"
    assert not modes & N.MB_T8X8, "MB_I8X8 beside MB_T8X8"
    assert all((mask >> (4 * k)) & 15 in (0, 15) for k in range(4)), "luma nibbles of %#x" % mask


def luma8x8_of(pic, m, refuse=True):
    """({quadrant k: r[8][8]} of the coded 8x8 blocks of the flagged macroblock m, the Range of everything bounded on the way)"""
    r = pic.mb_records()[m]
    check_record(r)
    out, rng = {}, Range()
    for k in range(4):
        if (int(r["coef_mask"]) >> (4 * k)) & 1:
            out[k] = T8.block8x8(T8.levels8_of(pic, r, k), int(r["qp"]), rng)
    if refuse and not rng.ok:
        raise OutOfRange("macroblock %d (Intra 8x8): %s outside -2^15 .. 2^15 - 1: H.264 defines no result" % (m, sorted(set(rng.bad))))
    return out, rng


class IntraChecker(intra_checker.IntraChecker):
    """intra_checker.IntraChecker with the Intra 8x8 macroblock"""
    census8 = None

    def _intra_mb(self, pic, m, F):
        r = pic.mb_records()[m]
        if not flagged(r):
            return super()._intra_mb(pic, m, F)
        d = pic.desc
        a = int(r["avail"])
        L, T, TR, TL = bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT), bool(a & N.AVAIL_TOPLEFT)
        x0, y0 = (m % d.mb_w) * 16, (m // d.mb_w) * 16
        Y = F[0]
        res, _ = luma8x8_of(pic, m)
        modes = pic.i4modes[m * 16:m * 16 + 16]
        for k in range(4):
            assert len(set(int(v) for v in modes[4 * k:4 * k + 4])) == 1, "macroblock %d: i4modes of 8x8 block %d are not one mode" % (m, k)
            x, y = x0 + (k & 1) * 8, y0 + (k >> 1) * 8
            o = predict_block(Y, x, y, int(modes[4 * k]), block_availability(k, L, T, TR, TL), self.census8, k)
            if k in res:
                o = np.clip(o + np.array(res[k], np.int64), 0, 255)
            Y[y:y + 8, x:x + 8] = o
        cx, cy = x0 // 2, y0 // 2
        cmode = (int(r["intra_modes"]) >> 4) & 3
        for ch in (1, 2):
            P = F[ch]
            left = P[cy:cy + 8, cx - 1].tolist() if L else None
            top = P[cy - 1, cx:cx + 8].tolist() if T else None
            corner = int(P[cy - 1, cx - 1]) if TL else None
            P[cy:cy + 8, cx:cx + 8] = intra_checker.pred_chroma(cmode, left, top, corner)
        for (plane, x, y), rr in T8.chroma_residual_of(pic, m).items():
            residual_checker.construct(F[plane], cx + x, cy + y, rr)


def deblock(pic, planes, tells=None):
    """t8x8_checker.deblock with the luma edges 1 and 3 of Intra 8x8 macroblocks skipped too: that walk asks one question of a record
    - does it carry N.MB_T8X8 - and nothing the filter calls reads intra_modes, so the Intra 8x8 records carry that bit for its
    duration"""
    rec = pic.mb_records()
    mine = np.flatnonzero((rec["intra_modes"] & N.MB_I8X8) != 0)
    rec["intra_modes"][mine] |= N.MB_T8X8
    try:
        return T8.deblock(pic, planes, tells)
    finally:
        rec["intra_modes"][mine] &= ~N.MB_T8X8 & 0xff


class SpecRecon(T8.SpecRecon):
    """t8x8_checker.SpecRecon for pictures whose I4x4 records may carry N.MB_I8X8"""

    def __init__(self, mb_w, mb_h, slots):
        super().__init__(mb_w, mb_h, slots)
        self.census8 = Census()
        self.intra = IntraChecker(None, mb_w, mb_h, slots, residual=spec_recon._Residual(), inter=self._inter, store=self.store)
        self.intra.census8 = self.census8
        self.met = 0                           # pictures with at least one Intra 8x8 macroblock

    def reconstruct(self, pic):
        self.met += bool((pic.mb_records()["intra_modes"] & N.MB_I8X8).any())
        F = self.nodeblock(pic)
        if pic.desc.deblock:
            deblock(pic, F, self.tells)
        return F
