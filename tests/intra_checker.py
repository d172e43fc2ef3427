"""Checker for intra prediction (TEST INFRASTRUCTURE), written from the text of H.264 8.3 - not from oracle/cpu_recon.c::recon_intra
and not from kernel_intra.h, which share one reading of the rules (and shared the reference's DC fall-back keyed on the top-left
flag, SURVEY A-Q7, until this checker showed it on multi-slice pictures).

Per picture:
1. the samples of the inter macroblocks: a copy of the picture in which EVERY intra macroblock (I_PCM included) is an inter
   macroblock with vector 0 and no residual goes through oracle_reconstruct_nodeblock (an I picture has none: step skipped);
   pictures with explicit weights first get their weighted predictions from wp_checker.WeightedChecker.predict, as in pcm_checker;
2. the intra macroblocks in raster order, in plain Python integers / numpy, straight into the picture: I_PCM samples are copied in
   place (8.3.5); Intra4x4 per block with the nine modes of 8.3.1.2 and the substitution of a missing top-right by p[3, -1];
   Intra16x16 (8.3.3) and chroma (8.3.4) with the DC rules by AVAILABILITY OF LEFT AND TOP.  Whether a neighbouring macroblock is
   available is the record's `avail` flag and nothing else (inside a macroblock: the decoding order of the 4x4 blocks, 6.4.11.4);
   a mode that reads an unavailable sample raises ValueError - never a substitute.
   The residual is not under test here (the known-answer files pin it to the reference): the oracle's kernel-level entry points
   do the arithmetic, on coefficient blocks found as include/p264hip.h lays them out ([luma DC][chroma DC][blocks 0..23 present]
   from coef_index, levels in zig-zag order, AC-only blocks in [0..14]);
3. oracle_deblock_picture on the picture's own records, as pcm_checker does.
On a single-slice picture this is oracle_reconstruct, byte for byte (tests/test_intra_checker_cpu.py).
The two things borrowed from the oracle - the inter macroblocks' samples of step 1 and the residual arithmetic of step 2 - are
pluggable (IntraChecker's `inter` and `residual`): tests/spec_recon.py plugs in tests/inter_checker.py and
tests/residual_checker.py, filters with tests/slice_filter_checker.py and needs no oracle at all."""
import ctypes as C

import numpy as np

from p264decoder_amd import _native as N
from tests import pcm_checker

# 4x4 luma blocks in decoding order -> position in units of blocks (6.4.3, figure 6-10)
BLK_X = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
BLK_Y = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]
BLK_AT = {(BLK_X[i], BLK_Y[i]): i for i in range(16)}
# zig-zag scan of a 4x4 block (table 8-13, frame macroblocks): scan position -> raster position y * 4 + x
ZIGZAG = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
# table 8-15: qPI -> QPC
CHROMA_QP = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
MODE4_NAMES = ("vertical", "horizontal", "DC", "diagonal down-left", "diagonal down-right", "vertical-right", "horizontal-down", "vertical-left", "horizontal-up")


class _Edge:
    """p[x, y] of 8.3.1.2 / 8.3.3 / 8.3.4: y = -1 is the row above (x = -1 the corner), x = -1 the column to the left.  left / top:
    sequences of ints or None, corner: int or None.  Reading a sample that is not available raises ValueError."""

    def __init__(self, left, top, corner, what):
        self.left, self.top, self.corner, self.what = left, top, corner, what

    def __call__(self, x, y):
        if x == -1 and y == -1:
            v = self.corner
        elif y == -1:
            v = None if self.top is None else self.top[x]
        else:
            assert x == -1
            v = None if self.left is None else self.left[y]
        if v is None:
            raise ValueError("%s reads p[%d, %d], which is not available" % (self.what, x, y))
        return int(v)


def top_with_topright(top4, topright4):
    """8.3.1.2: the eight samples p[0..7, -1].  When p[4..7, -1] are not available and p[0..3, -1] are, p[3, -1] stands in for them
    (and they count as available).  None when the row above is not available."""
    if top4 is None:
        return None
    t = [int(v) for v in top4]
    return t + ([int(v) for v in topright4] if topright4 is not None else [t[3]] * 4)


def dc_value(left, top, shift_both):
    """the four DC cases of 8.3.1.2.3 / 8.3.3.3 over n = len samples per side: both (sum + n) >> shift_both, one side
    (sum + n / 2) >> (shift_both - 1), none 128"""
    if left is not None and top is not None:
        return (sum(int(v) for v in left) + sum(int(v) for v in top) + (1 << (shift_both - 1))) >> shift_both
    one = left if left is not None else top
    if one is not None:
        return (sum(int(v) for v in one) + (1 << (shift_both - 2))) >> (shift_both - 1)
    return 128


def pred4x4(mode, left, top8, corner):
    """Intra4x4 prediction, 8.3.1.2.1-9.  left: p[-1, 0..3], top8: p[0..7, -1] (see top_with_topright), corner: p[-1, -1]; None =
    not available.  Returns int[4][4] indexed [y][x]."""
    if not 0 <= mode <= 8:
        raise ValueError("Intra4x4 mode %d" % mode)
    p = _Edge(left, top8, corner, "Intra4x4 %s" % MODE4_NAMES[mode])
    o = np.zeros((4, 4), np.int64)
    if mode == 2:
        o[:] = dc_value(left, None if top8 is None else top8[:4], 3)
        return o
    for y in range(4):
        for x in range(4):
            if mode == 0:
                v = p(x, -1)
            elif mode == 1:
                v = p(-1, y)
            elif mode == 3:
                v = (p(6, -1) + 3 * p(7, -1) + 2) >> 2 if x == 3 and y == 3 else (p(x + y, -1) + 2 * p(x + y + 1, -1) + p(x + y + 2, -1) + 2) >> 2
            elif mode == 4:
                if x > y:
                    v = (p(x - y - 2, -1) + 2 * p(x - y - 1, -1) + p(x - y, -1) + 2) >> 2
                elif x < y:
                    v = (p(-1, y - x - 2) + 2 * p(-1, y - x - 1) + p(-1, y - x) + 2) >> 2
                else:
                    v = (p(0, -1) + 2 * p(-1, -1) + p(-1, 0) + 2) >> 2
            elif mode == 5:
                z, k = 2 * x - y, x - (y >> 1)
                if z in (0, 2, 4, 6):
                    v = (p(k - 1, -1) + p(k, -1) + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p(k - 2, -1) + 2 * p(k - 1, -1) + p(k, -1) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(-1, y - 1) + 2 * p(-1, y - 2) + p(-1, y - 3) + 2) >> 2
            elif mode == 6:
                z, k = 2 * y - x, y - (x >> 1)
                if z in (0, 2, 4, 6):
                    v = (p(-1, k - 1) + p(-1, k) + 1) >> 1
                elif z in (1, 3, 5):
                    v = (p(-1, k - 2) + 2 * p(-1, k - 1) + p(-1, k) + 2) >> 2
                elif z == -1:
                    v = (p(-1, 0) + 2 * p(-1, -1) + p(0, -1) + 2) >> 2
                else:
                    v = (p(x - 1, -1) + 2 * p(x - 2, -1) + p(x - 3, -1) + 2) >> 2
            elif mode == 7:
                k = x + (y >> 1)
                v = (p(k, -1) + p(k + 1, -1) + 1) >> 1 if y in (0, 2) else (p(k, -1) + 2 * p(k + 1, -1) + p(k + 2, -1) + 2) >> 2
            else:
                z, k = x + 2 * y, y + (x >> 1)
                if z in (0, 2, 4):
                    v = (p(-1, k) + p(-1, k + 1) + 1) >> 1
                elif z in (1, 3):
                    v = (p(-1, k) + 2 * p(-1, k + 1) + p(-1, k + 2) + 2) >> 2
                elif z == 5:
                    v = (p(-1, 2) + 3 * p(-1, 3) + 2) >> 2
                else:
                    v = p(-1, 3)
            o[y, x] = v
    return o


def _plane(p, n, mul):
    """8.3.3.4 (n = 16: b = (5 H + 32) >> 6) and 8.3.4.4 for 4:2:0 (n = 8: b = (34 H + 32) >> 6)"""
    h = n // 2
    H = sum((i + 1) * (p(h + i, -1) - p(h - 2 - i, -1)) for i in range(h))
    V = sum((i + 1) * (p(-1, h + i) - p(-1, h - 2 - i)) for i in range(h))
    a = 16 * (p(-1, n - 1) + p(n - 1, -1))
    b, c = (mul * H + 32) >> 6, (mul * V + 32) >> 6
    o = np.zeros((n, n), np.int64)
    for y in range(n):
        for x in range(n):
            o[y, x] = min(max((a + b * (x - (h - 1)) + c * (y - (h - 1)) + 16) >> 5, 0), 255)
    return o


def pred16x16(mode, left, top, corner):
    """Intra16x16 prediction, 8.3.3.1-4: 0 vertical, 1 horizontal, 2 DC, 3 plane.  int[16][16] indexed [y][x]."""
    if not 0 <= mode <= 3:
        raise ValueError("Intra16x16 mode %d" % mode)
    p = _Edge(left, top, corner, "Intra16x16 %s" % ("vertical", "horizontal", "DC", "plane")[mode])
    o = np.zeros((16, 16), np.int64)
    if mode == 0:
        o[:] = [p(x, -1) for x in range(16)]
    elif mode == 1:
        o[:] = np.array([p(-1, y) for y in range(16)])[:, None]
    elif mode == 2:
        o[:] = dc_value(left, top, 5)
    else:
        o = _plane(p, 16, 5)
    return o


def pred_chroma(mode, left, top, corner):
    """intra chroma prediction of one 8x8 plane (4:2:0), 8.3.4.1-4: 0 DC, 1 horizontal, 2 vertical, 3 plane.  int[8][8] [y][x]."""
    if not 0 <= mode <= 3:
        raise ValueError("intra chroma mode %d" % mode)
    p = _Edge(left, top, corner, "intra chroma %s" % ("DC", "horizontal", "vertical", "plane")[mode])
    o = np.zeros((8, 8), np.int64)
    if mode == 1:
        o[:] = np.array([p(-1, y) for y in range(8)])[:, None]
    elif mode == 2:
        o[:] = [p(x, -1) for x in range(8)]
    elif mode == 3:
        o = _plane(p, 8, 34)
    else:
        for yO in (0, 4):
            for xO in (0, 4):
                t = None if top is None else [int(v) for v in top[xO:xO + 4]]
                l = None if left is None else [int(v) for v in left[yO:yO + 4]]
                if (xO, yO) == (0, 0) or (xO > 0 and yO > 0):      # 8.3.4.1: both, else the one that is there (top first), else 128
                    v = dc_value(l, t, 3) if (t is not None and l is not None) else dc_value(None, t, 3) if t is not None else dc_value(l, None, 3)
                elif xO > 0:                                       # 8.3.4.2: top if available, else left, else 128
                    v = dc_value(None, t, 3) if t is not None else dc_value(l, None, 3)
                else:                                              # 8.3.4.3: left if available, else top, else 128
                    v = dc_value(l, None, 3) if l is not None else dc_value(None, t, 3)
                o[yO:yO + 4, xO:xO + 4] = v
    return o


def block_availability(i, L, T, TR, TL):
    """(left, top, topright, corner) of 4x4 luma block i (decoding order) from the macroblock's four flags: a neighbouring block
    inside the macroblock is available when it precedes block i in decoding order, a place to the right of the macroblock in
    rows below its first never is (6.4.11.4, 6.4.12)"""
    bx, by = BLK_X[i], BLK_Y[i]
    left = bx > 0 or L
    top = by > 0 or T
    corner = True if (bx > 0 and by > 0) else T if bx > 0 else L if by > 0 else TL
    if by == 0:
        topright = T if bx < 3 else TR
    else:
        topright = bx < 3 and BLK_AT[(bx + 1, by - 1)] < i
    return bool(left), bool(top), bool(topright), bool(corner)


class IntraChecker:
    """a frame store of `slots` frames plus the scratch frame of the weighted checker; reconstruct() decodes one picture into it.
    self.dc_log: one entry per macroblock with LEFT and TOP and without TOPLEFT that predicts Intra16x16 DC or chroma DC -
    (macroblock, 'i16' / 'cb' / 'cr', mb_type, the DC of the standard, the DC of the left column alone)."""

    def __init__(self, oracle, mb_w, mb_h, slots, residual=None, inter=None, store=None):
        """residual: an object with the three hooks _luma4x4_residual / _luma16x16_residual / _chroma_residual (None: this
        object's, which call the oracle's entry points); inter: a callable (pic) that leaves the finished inter macroblocks of
        a P / B picture in store[dst_slot] (None: oracle_reconstruct_nodeblock on a flattened copy); store: the frame store,
        store[slot] = [y, u, v] (None: the weighted checker's).  With all three given no oracle handle is needed (oracle=None:
        tests/spec_recon.py); reconstruct()'s loop filter is the oracle's - such a caller filters nodeblock()'s result itself."""
        self.oracle = oracle
        if oracle is not None:
            self.pcm = pcm_checker.PcmChecker(oracle, mb_w, mb_h, slots)
            self.wp = self.pcm.wp
            self.store, self.s_slot = self.pcm.store, self.pcm.s_slot
        else:
            assert residual is not None and inter is not None and store is not None, "without an oracle every source must be given"
        if store is not None:
            self.store = store
        self.residual = self if residual is None else residual
        self.inter = self._oracle_inter if inter is None else inter
        self.dc_log = []

    # ---- the residual: arithmetic by the oracle's entry points, layout by include/p264hip.h ----
    def _block(self, pic, r, bit):
        mask = int(r["coef_mask"])
        if bit == N.COEF_LUMA_DC:
            k = 0
        elif bit == N.COEF_CHROMA_DC:
            k = 1 if mask & N.COEF_LUMA_DC else 0
        else:
            k = (1 if mask & N.COEF_LUMA_DC else 0) + (1 if mask & N.COEF_CHROMA_DC else 0) + bin(mask & (bit - 1) & 0xffffff).count("1")
        at = (int(r["coef_index"]) + k) * 16
        return pic.coefs[at:at + 16]

    def _add(self, plane, x, y, d):
        d = np.ascontiguousarray(d, np.int16)
        self.oracle.oracle_add4x4_idct(plane.ctypes.data + y * plane.shape[1] + x, plane.shape[1], d.ctypes.data)

    @staticmethod
    def _unscan(lv, ac):
        d = np.zeros(16, np.int16)
        if ac:
            d[ZIGZAG[1:]] = lv[:15]
        else:
            d[ZIGZAG] = lv
        return d

    def _luma4x4_residual(self, pic, r, Y, x, y, i):
        d = self._unscan(self._block(pic, r, 1 << i), False)
        self.oracle.oracle_dequant4x4(d.ctypes.data, int(r["qp"]))
        self._add(Y, x, y, d)

    def _luma16x16_residual(self, pic, r, Y, x0, y0):
        mask, qp = int(r["coef_mask"]), int(r["qp"])
        dc = self._unscan(self._block(pic, r, N.COEF_LUMA_DC), False) if mask & N.COEF_LUMA_DC else np.zeros(16, np.int16)
        self.oracle.oracle_idct4x4dc(dc.ctypes.data)
        self.oracle.oracle_dequant4x4_dc(dc.ctypes.data, qp)
        for i in range(16):
            d = np.zeros(16, np.int16)
            if mask >> i & 1:
                d = self._unscan(self._block(pic, r, 1 << i), True)
                self.oracle.oracle_dequant4x4(d.ctypes.data, qp)
            d[0] = dc[BLK_Y[i] * 4 + BLK_X[i]]
            self._add(Y, x0 + BLK_X[i] * 4, y0 + BLK_Y[i] * 4, d)

    def _chroma_residual(self, pic, r, planes, x0, y0):
        if not int(r["cbp"]) >> 4:
            return
        mask = int(r["coef_mask"])
        qpc = CHROMA_QP[min(max(int(r["qp"]) + pic.desc.chroma_qp_offset, 0), 51)]
        for ch in range(2):
            dc = np.zeros(4, np.int16)
            if mask & N.COEF_CHROMA_DC:
                dc[:] = self._block(pic, r, N.COEF_CHROMA_DC)[ch * 4:ch * 4 + 4]
            self.oracle.oracle_idct2x2dc(dc.ctypes.data)
            self.oracle.oracle_dequant2x2_dc(dc.ctypes.data, qpc)
            for i in range(4):
                b = 16 + ch * 4 + i
                d = np.zeros(16, np.int16)
                if mask >> b & 1:
                    d = self._unscan(self._block(pic, r, 1 << b), True)
                    self.oracle.oracle_dequant4x4(d.ctypes.data, qpc)
                d[0] = dc[i]
                self._add(planes[1 + ch], x0 + (i & 1) * 4, y0 + (i >> 1) * 4, d)

    # ---- step 2 for one macroblock ----
    def _intra_mb(self, pic, m, F):
        d = pic.desc
        r = pic.mb_records()[m]
        t = int(r["mb_type"])
        if t == N.MB_IPCM:
            raw = pic.coefs.view(np.uint8)
            at = int(r["coef_index"]) * 32
            pcm_checker.put_samples(F, d.mb_w, m, raw[at:at + 384])
            return
        a = int(r["avail"])
        L, T, TR, TL = bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT), bool(a & N.AVAIL_TOPLEFT)
        x0, y0 = (m % d.mb_w) * 16, (m // d.mb_w) * 16
        Y = F[0]
        quirk = L and T and not TL
        if t == N.MB_I16x16:
            left = Y[y0:y0 + 16, x0 - 1].tolist() if L else None
            top = Y[y0 - 1, x0:x0 + 16].tolist() if T else None
            corner = int(Y[y0 - 1, x0 - 1]) if TL else None
            mode = int(r["intra_modes"]) & 3
            Y[y0:y0 + 16, x0:x0 + 16] = pred16x16(mode, left, top, corner)
            if quirk and mode == 2:
                self.dc_log.append((m, "i16", t, dc_value(left, top, 5), dc_value(left, None, 5)))
            self.residual._luma16x16_residual(pic, r, Y, x0, y0)
        else:
            assert t == N.MB_I4x4, t
            for i in range(16):
                x, y = x0 + BLK_X[i] * 4, y0 + BLK_Y[i] * 4
                bl, bt, btr, bc = block_availability(i, L, T, TR, TL)
                left = Y[y:y + 4, x - 1].tolist() if bl else None
                top8 = top_with_topright(Y[y - 1, x:x + 4].tolist() if bt else None, Y[y - 1, x + 4:x + 8].tolist() if btr else None)
                corner = int(Y[y - 1, x - 1]) if bc else None
                Y[y:y + 4, x:x + 4] = pred4x4(int(pic.i4modes[m * 16 + i]), left, top8, corner)
                if int(r["coef_mask"]) >> i & 1:
                    self.residual._luma4x4_residual(pic, r, Y, x, y, i)
        cx, cy = x0 // 2, y0 // 2
        cmode = (int(r["intra_modes"]) >> 4) & 3
        for ch in (1, 2):
            P = F[ch]
            left = P[cy:cy + 8, cx - 1].tolist() if L else None
            top = P[cy - 1, cx:cx + 8].tolist() if T else None
            corner = int(P[cy - 1, cx - 1]) if TL else None
            o = pred_chroma(cmode, left, top, corner)
            P[cy:cy + 8, cx:cx + 8] = o
            if quirk and cmode == 0:
                self.dc_log.append((m, "cb" if ch == 1 else "cr", t, int(o[0, 0]), dc_value(left[:4], None, 3)))
        self.residual._chroma_residual(pic, r, F, cx, cy)

    def _oracle_inter(self, pic):
        """the samples of the inter macroblocks: a copy of the picture in which every intra macroblock is an inter macroblock with
        vector 0 and no residual, through oracle_reconstruct_nodeblock"""
        d = pic.desc
        rec = pic.mb_records()
        n = d.mb_w * d.mb_h
        intra = rec["mb_type"] <= N.MB_IPCM
        flat = pcm_checker._Copy(pic)
        if d.explicit_wp:
            self.wp.predict(pic)                           # the weighted predictions of the inter macroblocks into S ...
            flat.ref_idx[:] = 0                            # ... from where every macroblock of the copy takes them
            flat.mv[:] = 0
            flat.desc.ref_slot[0] = self.s_slot
            flat.desc.weighted_bipred = 0
            flat.desc.explicit_wp = 0
        else:
            flat.ref_idx[np.repeat(intra, 4)] = 0
            flat.mv[np.repeat(intra, 32)] = 0
        l1 = np.ones(n, bool) if d.explicit_wp else intra
        flat.ref_idx_l1[np.repeat(l1, 4)] = -1
        flat.mv_l1[np.repeat(l1, 32)] = 0
        flat.rec["mb_type"][intra] = N.MB_B if d.slice_type == N.SLICE_B else N.MB_P_L0
        flat.rec["coef_mask"][intra] = 0
        flat.rec["cbp"][intra] = 0
        self.oracle.oracle_reconstruct_nodeblock(C.byref(flat.desc), self.store.ptrs)

    def nodeblock(self, pic):
        """steps 1 and 2: the picture before the loop filter, in its frame of the store"""
        d = pic.desc
        intra = pic.mb_records()["mb_type"] <= N.MB_IPCM
        if d.slice_type == N.SLICE_I:
            assert intra.all(), "an I picture with inter macroblocks"
        else:
            self.inter(pic)
        F = self.store[d.dst_slot]
        for m in np.flatnonzero(intra):
            self._intra_mb(pic, int(m), F)
        return F

    def reconstruct(self, pic):
        """the decoded picture (views into the store)"""
        d = pic.desc
        self.nodeblock(pic)
        if d.deblock:
            self.oracle.oracle_deblock_picture(C.byref(pic.desc), self.store.ptrs)
        return self.store[d.dst_slot]


# ---- what a picture's intra macroblocks exercise (for coverage assertions; computed from the records alone) ----
def survey(pic, seen, dense):
    """raises the sets of `seen` (a dict, created empty by new_survey): dense = the picture is decoded by the dense k_intra launch
    (an I picture in the batch), else by k_intra_sparse - the road of pcm_checker.sparse_roads is recorded with each flag set"""
    rec = pic.mb_records()
    roads = None if dense else pcm_checker.sparse_roads(pic)
    for m in np.flatnonzero(rec["mb_type"] <= N.MB_IPCM):
        m = int(m)
        t, a = int(rec["mb_type"][m]), int(rec["avail"][m])
        L, T, TR = bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT)
        seen["avail"].add((t, "dense" if dense else int(roads[m]), a))
        if t == N.MB_IPCM:
            continue
        if (int(rec["intra_modes"][m]) >> 4) & 3 == 0:
            seen["chroma_dc"].add((L, T))
        if t == N.MB_I16x16:
            if int(rec["intra_modes"][m]) & 3 == 2:
                seen["i16_dc"].add((L, T))
            continue
        modes = pic.i4modes[m * 16:m * 16 + 16]
        if modes[0] == 2:
            seen["i4_block0_dc"].add((L, T))
        if T and not TR and modes[5] in (3, 7):
            seen["i4_tr_missing_mb"].add(int(modes[5]))
        for i in (3, 7, 11, 13, 15):
            if modes[i] in (3, 7):
                seen["i4_tr_missing_inside"].add(int(modes[i]))
    return seen


def new_survey():
    return dict(avail=set(), chroma_dc=set(), i16_dc=set(), i4_block0_dc=set(), i4_tr_missing_mb=set(), i4_tr_missing_inside=set())
