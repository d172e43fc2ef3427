"""The drawn batches behind tests/test_gpu_ipcm_seam_fuzz.py and its CPU twins: per family three pictures of seam_fuzz.make_picture
with a share of their macroblocks turned into I_PCM records, the frames of tests/pcm_checker.py, and the coverage figures."""
import ctypes as C

import numpy as np

from p264decoder_amd import _native as N
from tests import pcm_checker, pcm_fuzz, seam_fuzz

SLOTS, DST, S = 3, 2, 3
CONFIGS = {
    # name: (mb_w, mb_h, I_PCM share, samples, make_picture keywords)
    "p_2pct": (12, 9, 0.02, "noise", dict(n_ref=2)),
    "p_30pct": (12, 9, 0.30, "noise", dict(n_ref=2, slices=2)),
    "p_100pct": (9, 7, 1.00, "extremes", dict(n_ref=1)),
    "b_30pct": (12, 9, 0.30, "noise", dict(n_ref=2, n_ref_l1=2, b_picture=True)),
    "b_100pct": (9, 7, 1.00, "noise", dict(n_ref=2, n_ref_l1=1, b_picture=True)),
    "b_weighted": (9, 7, 0.30, "noise", dict(n_ref=2, n_ref_l1=2, b_picture=True, explicit_wp="legal")),
    # smooth samples next to neighbours of QP 46 with both offsets + 6: the mean with the I_PCM macroblock's QP 0 is 23, index 29 -
    # the filter works on these edges, and changes samples inside the I_PCM macroblocks
    "p_smooth_hiqp": (12, 9, 0.30, "frame", dict(n_ref=1, qp_mode=46, mv_range=0, level_style="small")),
    "b_smooth_hiqp": (10, 8, 0.30, "frame", dict(n_ref=1, n_ref_l1=1, b_picture=True, qp_mode=46, mv_range=0, level_style="small")),
    "p_slices_idc012": (10, 8, 0.30, "noise", dict(n_ref=2, slices=3, slice_idcs=[0, 1, 2])),
    "p_single_row": (11, 1, 0.30, "noise", dict(n_ref=1, slices=2)),
    "p_single_column": (1, 9, 0.30, "noise", dict(n_ref=1, slices=2)),
    "p_wide_67": (67, 3, 0.30, "noise", dict(n_ref=2)),
}


def prepare(oracle, name, with_i):
    """the batch of a family: [(picture, its reference frames, the checker's frame)] per stream, and what the pictures contain"""
    mb_w, mb_h, share, samples, kw = CONFIGS[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 131 + with_i)
    smooth = samples == "frame"
    batch, seen = [], dict(roads=set(), kinds=set(), luma=0, chroma=0, i4tr=0, n_pcm=0, qps=set())
    oracle.oracle_stats_reset()
    for s in range(S):
        chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, SLOTS)
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if smooth else "noise")
        for slot in range(DST):
            for dst, src in zip(chk.store[slot], f):
                dst[:] = src
        is_i = with_i and s == S - 1
        k = dict(kw)
        if is_i:
            k = {a: b for a, b in k.items() if a not in ("b_picture", "n_ref_l1", "explicit_wp")}
        k.setdefault("level_style", "mixed"); k.setdefault("qp_mode", "random")
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=not is_i, slots=SLOTS, dst_slot=DST, intra_share=0.15, **k)
        if smooth:
            pic.desc.alpha_c0_offset = pic.desc.beta_offset = 6
        pcm_fuzz.to_ipcm(rng, pic, share, samples=samples, src=f)
        refs = [[a.copy() for a in chk.store[slot]] for slot in range(DST)]
        stats = {}
        want = [a.copy() for a in chk.reconstruct(pic, stats)]
        rec = pic.rec
        pcm = rec["mb_type"] == N.MB_IPCM
        seen["n_pcm"] += int(pcm.sum())
        seen["luma"] += stats.get("pcm_luma_filtered", 0); seen["chroma"] += stats.get("pcm_chroma_filtered", 0)
        seen["kinds"] |= pcm_fuzz.neighbour_kinds(pic)
        seen["i4tr"] += pcm_fuzz.i4_topright_from_ipcm(pic)
        seen["qps"] |= set(rec["qp"][~pcm].tolist())
        if not is_i:
            seen["roads"] |= set(pcm_checker.sparse_roads(pic)[pcm].tolist())
        batch.append((pic, refs, want))
    st = (C.c_longlong * 8)()
    oracle.oracle_stats_get(st)
    seen["mean_qp_edges"] = int(st[6])                      # edges the oracle's loop filter took with the mean of two different QPs
    return batch, seen


def check_coverage(name, with_i, seen):
    mb_w, mb_h, share, samples, kw = CONFIGS[name]
    assert seen["n_pcm"] >= max(1, int(0.5 * share * mb_w * mb_h * S)), seen["n_pcm"]
    if name in ("p_30pct", "b_30pct") and not with_i:
        assert seen["roads"] == {0, 1, 2}, "not every road of the sparse path met an I_PCM macroblock: %s" % seen["roads"]
    if name in ("p_30pct", "b_30pct"):
        want = {(d, k) for d in ("left", "top", "topleft", "topright") for k in ("i4", "i16", "ipcm", "inter")}
        assert seen["kinds"] == want, sorted(want - seen["kinds"])
        assert seen["i4tr"] > 0, "no Intra4x4 block predicts from the samples of an I_PCM macroblock above and to the right"
        assert min(seen["qps"]) <= 2 and max(seen["qps"]) >= 49          # QP 0 (the I_PCM records) meets QP 51 and everything between
        assert seen["mean_qp_edges"] > 0
    if samples == "frame":
        assert seen["luma"] > 0 and seen["chroma"] > 0, "the loop filter changed no sample inside an I_PCM macroblock: %s" % seen
