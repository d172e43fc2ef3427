"""Checker for pictures with explicit weighted prediction (TEST INFRASTRUCTURE, built on the CPU oracle, which knows no weights).

Per picture:
1. every inter 4x4 block's prediction from each list it uses, out of oracle_mc_luma / oracle_mc_chroma on the checker's own
   reference planes, weighted with H.264 8.4.2.3.2 in numpy and written into a scratch frame S;
2. a copy of the picture in which every inter macroblock predicts from list 0, index 0, vector 0 (B pictures: list 1 unused),
   list 0's entry 0 being S - residual and intra macroblocks unchanged - through oracle_reconstruct_nodeblock: the weighted
   prediction plus the residual, in that order;
3. oracle_deblock_picture on the picture's own records, vectors and indices (it tells reference pictures apart by their frame,
   H.264 8.7.2.1, in P and B pictures alike - tests/deblock_checker.py holds it to that).
With identity tables (weight 2^denom, offset 0) this is oracle_reconstruct bit for bit (tests/test_weighted_pred_cpu.py)."""
import ctypes as C

import numpy as np

from p264decoder_amd import _native as N
from tests import oracle_bind


def _bind(oracle):
    for f in ("oracle_mc_luma", "oracle_mc_chroma"):
        getattr(oracle, f).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        getattr(oracle, f).restype = None


def _weigh(p0, p1, use0, use1, e0, e1, d, stats=None):
    """8.4.2.3.2; p0 / p1 int64 arrays (None where the list is unused), e = (weight, offset).  stats: a dict whose counters
    'clip_low' / 'clip_high' (samples the final Clip1 moved) and 'bi_past_limit' (bi-predicted blocks whose weight sum is outside
    -128 .. (d == 7 ? 127 : 128)) are raised"""
    if use0 and use1:
        v = ((p0 * e0[0] + p1 * e1[0] + (1 << d)) >> (d + 1)) + ((e0[1] + e1[1] + 1) >> 1)
    else:
        p, (w, o) = (p0, e0) if use0 else (p1, e1)
        v = (((p * w + (1 << (d - 1))) >> d) + o) if d >= 1 else p * w + o
    if stats is not None:
        stats["clip_low"] = stats.get("clip_low", 0) + int((v < 0).sum())
        stats["clip_high"] = stats.get("clip_high", 0) + int((v > 255).sum())
        if use0 and use1 and not -128 <= int(e0[0]) + int(e1[0]) <= (127 if d == 7 else 128):
            stats["bi_past_limit"] = stats.get("bi_past_limit", 0) + 1
    return np.clip(v, 0, 255).astype(np.uint8)


class _Copy:
    """an owned copy of a picture's descriptor and arrays (what the oracle reads)"""

    def __init__(self, pic):
        n = pic.desc.mb_w * pic.desc.mb_h
        d = N.Picture()
        C.memmove(C.byref(d), C.byref(pic.desc), C.sizeof(N.Picture))
        self.mv = pic.mv.copy()
        self.ref_idx = pic.ref_idx.copy()
        self.is_b = d.slice_type == N.SLICE_B
        self.mv_l1 = pic.mv_l1.copy() if self.is_b else np.zeros(n * 32, np.int16)
        self.ref_idx_l1 = pic.ref_idx_l1.copy() if self.is_b else np.full(n * 4, -1, np.int8)
        d.mv = C.cast(self.mv.ctypes.data, C.POINTER(C.c_int16))
        d.ref_idx = C.cast(self.ref_idx.ctypes.data, C.POINTER(C.c_int8))
        if self.is_b:
            d.mv_l1 = C.cast(self.mv_l1.ctypes.data, C.POINTER(C.c_int16))
            d.ref_idx_l1 = C.cast(self.ref_idx_l1.ctypes.data, C.POINTER(C.c_int8))
        self.desc = d


class WeightedChecker:
    """a frame store of `slots` frames plus the scratch frame S; reconstruct() decodes one parsed picture into it"""

    def __init__(self, oracle, mb_w, mb_h, slots):
        _bind(oracle)
        self.oracle = oracle
        self.s_slot = slots
        self.store = oracle_bind.FrameStore(mb_w, mb_h, slots + 1)

    def _mc(self, slot, c, x, y, mvx, mvy, n):
        plane = self.store[slot][c]
        h, w = plane.shape
        out = np.empty((n, n), np.uint8)
        fn = self.oracle.oracle_mc_luma if c == 0 else self.oracle.oracle_mc_chroma
        fn(plane.ctypes.data, w, h, x, y, mvx, mvy, n, n, out.ctypes.data, n)
        return out.astype(np.int64)

    def predict(self, pic, stats=None):
        """step 1: the weighted predictions of every inter block into S (stats: see _weigh)"""
        d = pic.desc
        is_b = d.slice_type == N.SLICE_B
        recs = pic.mb_records()
        tab = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2).astype(np.int64)
        S = self.store[self.s_slot]
        for m in range(d.mb_w * d.mb_h):
            if int(recs["mb_type"][m]) <= N.MB_IPCM:
                continue
            mbx, mby = m % d.mb_w, m // d.mb_w
            for b in range(16):
                bx, by = b & 3, b >> 2
                q = (by >> 1) * 2 + (bx >> 1)
                r0 = int(pic.ref_idx[m * 4 + q])
                r1 = int(pic.ref_idx_l1[m * 4 + q]) if is_b else -1
                use1 = r1 >= 0
                use0 = r0 >= 0 or not use1
                i0 = r0 if 0 <= r0 < d.n_ref else 0                 # (negative or past the list: entry 0, include/p264hip.h)
                i1 = r1 if use1 and r1 < d.n_ref_l1 else 0
                X, Y = mbx * 16 + bx * 4, mby * 16 + by * 4
                v0 = pic.mv[(m * 16 + b) * 2:(m * 16 + b) * 2 + 2]
                v1 = pic.mv_l1[(m * 16 + b) * 2:(m * 16 + b) * 2 + 2] if is_b else (0, 0)
                for c in range(3):
                    n, x, y = (4, X, Y) if c == 0 else (2, X // 2, Y // 2)
                    p0 = self._mc(d.ref_slot[i0], c, x, y, int(v0[0]), int(v0[1]), n) if use0 else None
                    p1 = self._mc(d.ref_slot_l1[i1], c, x, y, int(v1[0]), int(v1[1]), n) if use1 else None
                    S[c][y:y + n, x:x + n] = _weigh(p0, p1, use0, use1, tab[0, i0, c], tab[1, i1, c], d.wp_log2_denom[min(c, 1)], stats)

    def reconstruct(self, pic, stats=None):
        """the picture as a decoder with explicit weights makes it; returns its planes (views into the store)"""
        d = pic.desc
        if not d.explicit_wp:
            return oracle_bind.reconstruct(self.oracle, self.store, pic)
        self.predict(pic, stats)
        # step 2: list 0, index 0 = S, vector 0, for every inter macroblock
        flat = _Copy(pic)
        inter = np.repeat(pic.mb_records()["mb_type"] > N.MB_IPCM, 4)
        flat.ref_idx[inter] = 0
        flat.mv[np.repeat(inter, 8)] = 0
        flat.ref_idx_l1[:] = -1
        flat.mv_l1[:] = 0
        flat.desc.ref_slot[0] = self.s_slot
        flat.desc.weighted_bipred = 0
        self.oracle.oracle_reconstruct_nodeblock(C.byref(flat.desc), self.store.ptrs)
        # step 3: the loop filter with the picture's own motion
        if d.deblock:
            self.oracle.oracle_deblock_picture(C.byref(pic.desc), self.store.ptrs)
        return self.store[d.dst_slot]
