"""Checker for pictures with I_PCM macroblocks (TEST INFRASTRUCTURE, built on the CPU oracle, which knows no I_PCM and stays as
it is: an inter macroblock with vector 0 and no residual copies its reference samples exactly, and the oracle's reconstruction
and its loop filter can be called separately).

Per picture:
1. the samples of every I_PCM macroblock (the twelve blocks of coefs[] at its coef_index: 256 luma, 64 Cb, 64 Cr) are written
   into a scratch frame S of the checker's frame store, at the macroblock's own position;
2. a copy of the picture in which every I_PCM macroblock is an inter macroblock (P264_MB_P_L0; P264_MB_B with list 1 unused in a
   B picture; an I picture's copy is a P picture) with vector 0, coef_mask 0, cbp 0 and a list-0 index appended behind the
   picture's own list, whose slot is S, goes through oracle_reconstruct_nodeblock - the samples are in place when the macroblocks
   to the right and below predict from them; availability flags untouched;
3. oracle_deblock_picture with the picture's ORIGINAL records: type 2 is intra to it, and qp 0 is what H.264 8.7.2.2 asks for.
A picture with sixteen list-0 entries has no room for S and is refused.  Pictures with explicit weights compose with
wp_checker.WeightedChecker.predict: its scratch frame takes the I_PCM samples as well, and step 2 flattens both kinds.
Without an I_PCM macroblock this is oracle_reconstruct (or the weighted checker) itself."""
import ctypes as C

import numpy as np

from p264decoder_amd import _native as N
from tests import oracle_bind, wp_checker

IPCM_MASK = 0x00000fff


def ipcm_samples(pic):
    """[(macroblock index, uint8[384])] of a picture (parsed or built at the seam)"""
    raw = pic.coefs.view(np.uint8)
    r = pic.mb_records()
    return [(int(m), raw[int(r["coef_index"][m]) * 32:int(r["coef_index"][m]) * 32 + 384]) for m in np.flatnonzero(r["mb_type"] == N.MB_IPCM)]


def put_samples(frame, mb_w, m, s):
    """384 sample bytes into planes (Y, U, V) at macroblock m"""
    x, y = (m % mb_w) * 16, (m // mb_w) * 16
    frame[0][y:y + 16, x:x + 16] = s[:256].reshape(16, 16)
    frame[1][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = s[256:320].reshape(8, 8)
    frame[2][y // 2:y // 2 + 8, x // 2:x // 2 + 8] = s[320:384].reshape(8, 8)


def get_samples(frame, mb_w, m):
    x, y = (m % mb_w) * 16, (m // mb_w) * 16
    return np.concatenate([frame[0][y:y + 16, x:x + 16].reshape(-1), frame[1][y // 2:y // 2 + 8, x // 2:x // 2 + 8].reshape(-1),
                           frame[2][y // 2:y // 2 + 8, x // 2:x // 2 + 8].reshape(-1)])


class _Copy(wp_checker._Copy):
    """... and of its records"""

    def __init__(self, pic):
        super().__init__(pic)
        self.rec = pic.mb_records().copy()
        self.desc.mb = C.cast(self.rec.ctypes.data, C.POINTER(N.MbInfo))


def sparse_roads(pic):
    """Which road of k_intra_sparse (kernel_intra.h, K3) every intra macroblock of a P / B picture takes, from the picture's intra
    mask alone: 0 / 1 = ready in round 0 / 1 (no pending intra macroblock to the left, above-left, above, above-right; the ready
    ones leave the pending set between the rounds), 2 = left to the ordered band walk.  int8[n_mb], -1 for inter macroblocks.
    (The lists take 256 macroblocks per type and round; what they cannot take stays pending - not modelled: small pictures.)"""
    w, h = pic.mb_w, pic.mb_h
    pend = (pic.mb_records()["mb_type"] <= N.MB_IPCM).reshape(h, w).copy()
    road = np.full((h, w), -1, np.int8)
    for rnd in range(2):
        p = np.pad(pend, 1)
        blocked = p[1:-1, :-2] | p[:-2, :-2] | p[:-2, 1:-1] | p[:-2, 2:]
        ready = pend & ~blocked
        road[ready] = rnd
        pend &= ~ready
    road[pend] = 2
    return road.reshape(-1)


class PcmChecker:
    """a frame store of `slots` frames plus the scratch frame S; reconstruct() decodes one picture into it"""

    def __init__(self, oracle, mb_w, mb_h, slots):
        self.oracle = oracle
        self.wp = wp_checker.WeightedChecker(oracle, mb_w, mb_h, slots)
        self.store, self.s_slot = self.wp.store, self.wp.s_slot
        self.last_nodeblock = None

    def nodeblock(self, pic):
        """steps 1 and 2: the picture before the loop filter, in its frame of the store"""
        d = pic.desc
        rec = pic.mb_records()
        pcm = rec["mb_type"] == N.MB_IPCM
        if not pcm.any() and not d.explicit_wp:
            return oracle_bind.reconstruct(self.oracle, self.store, pic, deblock=False)
        if pcm.any() and d.slice_type != N.SLICE_I and d.n_ref >= N.MAX_REFS:
            raise ValueError("pcm_checker: the picture's list 0 has %d entries, no room for the scratch frame" % d.n_ref)
        assert (rec["coef_mask"][pcm] == IPCM_MASK).all() and (rec["qp"][pcm] == 0).all(), "not the I_PCM record of include/p264hip.h"
        flat = _Copy(pic)
        if d.explicit_wp:
            self.wp.predict(pic)                               # the weighted predictions of the real inter macroblocks into S ...
            inter = np.repeat(rec["mb_type"] > N.MB_IPCM, 4)
            flat.ref_idx[inter] = 0                            # ... which then copy them from entry 0 = S
            flat.mv[np.repeat(inter, 8)] = 0
            flat.ref_idx_l1[:] = -1
            flat.mv_l1[:] = 0
            flat.desc.ref_slot[0] = self.s_slot
            flat.desc.weighted_bipred = 0
            flat.desc.explicit_wp = 0
            s_index = 0
        else:
            s_index = d.n_ref if d.slice_type != N.SLICE_I else 0
            flat.desc.n_ref = s_index + 1
            flat.desc.ref_slot[s_index] = self.s_slot
        for m, s in ipcm_samples(pic):
            put_samples(self.store[self.s_slot], d.mb_w, m, s)
        if d.slice_type == N.SLICE_I:
            flat.desc.slice_type = N.SLICE_P
        flat.rec["mb_type"][pcm] = N.MB_B if d.slice_type == N.SLICE_B else N.MB_P_L0
        flat.rec["coef_mask"][pcm] = 0
        flat.rec["cbp"][pcm] = 0
        p4 = np.repeat(pcm, 4)
        flat.ref_idx[p4] = s_index
        flat.mv[np.repeat(pcm, 32)] = 0
        flat.ref_idx_l1[p4] = -1
        flat.mv_l1[np.repeat(pcm, 32)] = 0
        self.oracle.oracle_reconstruct_nodeblock(C.byref(flat.desc), self.store.ptrs)
        return self.store[d.dst_slot]

    def reconstruct(self, pic, stats=None):
        """the decoded picture (views into the store).  stats: a dict whose 'pcm_luma_filtered' / 'pcm_chroma_filtered' (samples
        inside I_PCM macroblocks that the loop filter changed) are raised"""
        d = pic.desc
        pcm = pic.mb_records()["mb_type"] == N.MB_IPCM
        if not pcm.any():
            return self.wp.reconstruct(pic)
        before = [a.copy() for a in self.nodeblock(pic)]
        self.last_nodeblock = before
        if d.deblock:
            self.oracle.oracle_deblock_picture(C.byref(pic.desc), self.store.ptrs)
        out = self.store[d.dst_slot]
        if stats is not None:
            ym = np.kron(pcm.reshape(d.mb_h, d.mb_w), np.ones((16, 16), bool))
            cm = np.kron(pcm.reshape(d.mb_h, d.mb_w), np.ones((8, 8), bool))
            stats["pcm_luma_filtered"] = stats.get("pcm_luma_filtered", 0) + int(((out[0] != before[0]) & ym).sum())
            stats["pcm_chroma_filtered"] = stats.get("pcm_chroma_filtered", 0) + int((((out[1] != before[1]) | (out[2] != before[2])) & cm).sum())
        return out
