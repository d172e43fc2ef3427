"""I_PCM macroblocks at the CPU->GPU seam, on top of seam_fuzz.make_picture (TEST INFRASTRUCTURE): a drawn share of a picture's
macroblocks - intra and inter alike - becomes I_PCM records as include/p264hip.h defines them, and coefs[] / coef_index are
rebuilt around their twelve sample blocks."""
import numpy as np

from p264decoder_amd import _native as N
from tests import pcm_checker

IPCM_MASK = pcm_checker.IPCM_MASK


def to_ipcm(rng, pic, share, samples="noise", src=None, chosen=None, noise=1):
    """Convert macroblocks of a sealed seam_fuzz.SeamPicture in place; returns the picture.  share: probability per macroblock
    (chosen: a bool mask instead).  samples: 'noise' random bytes; 'extremes' runs of 0 / 255 / 128; 'frame' the samples of the
    planes `src` (Y, U, V) at the macroblock's position plus -noise .. noise (smooth content next to whatever the neighbours predict from
    the same frame: edges the loop filter works on)."""
    n = pic.n_mb
    rec = pic.rec
    if chosen is None:
        chosen = rng.random(n) < share
    old = pic.coefs.reshape(-1, 16)
    blocks = []
    at = 0
    for m in range(n):
        r = rec[m]
        if chosen[m]:
            if samples == "noise":
                s = rng.integers(0, 256, size=384, dtype=np.uint8)
            elif samples == "extremes":
                s = np.repeat(rng.choice(np.array([0, 255, 128], np.uint8), size=96), 4)
            else:
                s = np.clip(pcm_checker.get_samples(src, pic.mb_w, m).astype(int) + (rng.integers(-noise, noise + 1, size=384) if noise else 0), 0, 255).astype(np.uint8)
            r["mb_type"], r["qp"], r["cbp"], r["intra_modes"], r["flags"] = N.MB_IPCM, 0, 0, 0, 0
            r["coef_mask"], r["coef_index"] = IPCM_MASK, at
            blocks.append(s.view(np.int16).reshape(12, 16))
            at += 12
            pic.ref_idx[m * 4:m * 4 + 4] = -1
            pic.ref_idx_l1[m * 4:m * 4 + 4] = -1
            pic.mv[m * 32:m * 32 + 32] = 0
            pic.mv_l1[m * 32:m * 32 + 32] = 0
            pic.i4modes[m * 16:m * 16 + 16] = 2
        else:
            k = bin(int(r["coef_mask"]) & 0x3ffffff).count("1")
            if k:
                blocks.append(old[int(r["coef_index"]):int(r["coef_index"]) + k])
            r["coef_index"] = at
            at += k
    pic.coefs = np.ascontiguousarray(np.concatenate(blocks).reshape(-1), np.int16) if blocks else np.zeros(16, np.int16)
    pic.desc.n_coef_blocks = at
    return pic.seal()


def neighbour_kinds(pic):
    """{(direction, kind)} over the I_PCM macroblocks of a picture: direction in left / top / topleft / topright, kind in i4 / i16 /
    ipcm / inter - what the macroblock at that place is (picture borders aside)"""
    w, h = pic.mb_w, pic.mb_h
    t = pic.mb_records()["mb_type"].reshape(h, w)
    kind = {N.MB_I4x4: "i4", N.MB_I16x16: "i16", N.MB_IPCM: "ipcm"}
    out = set()
    for y, x in zip(*np.nonzero(t == N.MB_IPCM)):
        for name, (dy, dx) in (("left", (0, -1)), ("top", (-1, 0)), ("topleft", (-1, -1)), ("topright", (-1, 1))):
            if 0 <= y + dy and 0 <= x + dx < w:
                out.add((name, kind.get(int(t[y + dy, x + dx]), "inter")))
    return out


def i4_topright_from_ipcm(pic):
    """Intra4x4 macroblocks whose block 5 (the top-right 4x4) predicts down-left / vertical-left from the samples of an I_PCM
    macroblock above and to the right"""
    w = pic.mb_w
    rec = pic.mb_records()
    k = 0
    for m in np.flatnonzero(rec["mb_type"] == N.MB_I4x4):
        if rec["avail"][m] & N.AVAIL_TOPRIGHT and rec["mb_type"][m - w + 1] == N.MB_IPCM and int(pic.i4modes[m * 16 + 5]) in (3, 7):
            k += 1
    return k
