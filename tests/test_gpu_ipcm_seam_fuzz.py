"""I_PCM macroblocks at the seam on the MI355X: pictures of seam_fuzz.make_picture with a share of their macroblocks turned into
I_PCM records (tests/pcm_fuzz.py), through p264hip_reconstruct in batches of three streams, against tests/pcm_checker.py - bytes
of whole planes, every picture.  Every family runs once as a batch of P / B pictures only (k_intra_sparse; plain P batches carry
the fused edge-info role) and once with an I picture in the batch (k_intra), and goes into its input slots by one of the four
roads (plain upload, packed, compact, reserve / commit).  The coverage figures are computed on the CPU by `prepare`, so they can
be tried without a device.  All of this fails without the feature: the parent's kernels run an I_PCM record as Intra4x4."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from p264decoder_amd.recon import P264Error
from tests import pcm_checker, pcm_fuzz, seam_fuzz
from tests.test_gpu_seam_fuzz import compare

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
ROADS = ("upload", "packed", "compact", "commit")


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


def put(hip, lib, slot, pic, road):
    if road == "upload":
        hip.upload(slot, [pic])
    elif road == "packed":
        hip.upload_packed(slot, pic, HipReconstructor.pack(pic, lib))
    elif road == "compact":
        hip.upload_compact(slot, pic, HipReconstructor.pack_compact(pic, lib))
    else:
        blk = HipReconstructor.pack(pic, lib)
        dev, n = hip.input_reserve(slot, pic)
        assert n == blk.size and lib.p264hip_copy_to_device(dev, blk.ctypes.data, n) == 0
        hip.input_commit(slot)


@pytest.mark.gpu
@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_ipcm_seam_fuzz(lib, oracle, name, with_i):
    mb_w, mb_h, share, samples, kw = CONFIGS[name]
    batch, seen = prepare(oracle, name, with_i)
    hip = HipReconstructor(mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S, lib=lib)
    road = ROADS[(list(CONFIGS).index(name) + with_i) % 4]
    for s, (pic, refs, want) in enumerate(batch):
        for slot in range(DST):
            hip.write_frame(s, slot, *refs[slot])
        put(hip, lib, s, pic, road)
    hip.reconstruct(list(range(S)), list(range(S)))
    li = hip.last_launch()
    plain_p = not with_i and not kw.get("b_picture") and not kw.get("explicit_wp")
    assert (li["edge_info_fused"] > 0) == plain_p, li       # (fused edge info = the k_intra_sparse launch of a plain P batch)
    for s, (pic, refs, want) in enumerate(batch):
        compare(hip.read_frame(s, DST), want, "%s stream %d by %s" % (name, s, road), pic)
    hip.close()
    check_coverage(name, with_i, seen)


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


def test_coverage_of_the_drawn_batches(oracle):
    """(CPU) the same figures without a device"""
    for name in CONFIGS:
        for with_i in (False, True):
            check_coverage(name, with_i, prepare(oracle, name, with_i)[1])


@pytest.mark.gpu
def test_ipcm_1080p_batch(lib, oracle):
    rng = np.random.default_rng(1080)
    mb_w, mb_h = 120, 68
    hip = HipReconstructor(mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S, lib=lib)
    batch = []
    for s, (kw, share) in enumerate([(dict(n_ref=2), 0.03), (dict(n_ref=2, n_ref_l1=2, b_picture=True), 0.3), (dict(n_ref=1), 1.0)]):
        chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, SLOTS)
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "noise")
        for slot in range(DST):
            for dst, src in zip(chk.store[slot], f):
                dst[:] = src
            hip.write_frame(s, slot, *f)
        pic = pcm_fuzz.to_ipcm(rng, seam_fuzz.make_picture(rng, mb_w, mb_h, slots=SLOTS, dst_slot=DST, intra_share=0.1, level_style="small", **kw), share)
        batch.append((pic, [a.copy() for a in chk.reconstruct(pic)]))
        put(hip, lib, s, pic, ("upload", "compact", "packed")[s])
    hip.reconstruct(list(range(S)), list(range(S)))
    for s, (pic, want) in enumerate(batch):
        compare(hip.read_frame(s, DST), want, "1080p stream %d" % s, pic)
    hip.close()


@pytest.mark.gpu
def test_a_committed_ipcm_record_with_a_short_mask_is_refused(lib, oracle):
    """mask 0x7ff on an I_PCM record in the middle of the picture (more than twelve blocks of coefs[] behind its coef_index: even a
    kernel that ran it unchecked would read inside the slot): p264hip_reconstruct says P264HIP_EINVAL, and the context decodes a
    good picture right afterwards"""
    rng = np.random.default_rng(4242)
    mb_w, mb_h = 9, 7
    chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, SLOTS)
    hip = HipReconstructor(mb_w, mb_h, n_streams=1, slots=SLOTS, max_pictures=2, lib=lib)
    f = seam_fuzz.random_frame(rng, mb_w, mb_h, "noise")
    for slot in range(DST):
        for dst, src in zip(chk.store[slot], f):
            dst[:] = src
        hip.write_frame(0, slot, *f)
    pic = pcm_fuzz.to_ipcm(rng, seam_fuzz.make_picture(rng, mb_w, mb_h, n_ref=2, slots=SLOTS, dst_slot=DST), 0.4)
    good = HipReconstructor.pack(pic, lib)
    pcm = np.flatnonzero(pic.rec["mb_type"] == N.MB_IPCM)
    m = int(pcm[len(pcm) // 2])
    assert int(pic.rec["coef_index"][m]) + 24 <= pic.desc.n_coef_blocks
    lay = N.InputLayout()
    assert lib.p264hip_input_layout(C.byref(pic.desc), C.byref(lay)) == 0
    bad = good.copy()
    bad[lay.off_mb + 16 * m + 4:lay.off_mb + 16 * m + 8] = np.frombuffer(np.uint32(0x7ff).tobytes(), np.uint8)
    dev, n = hip.input_reserve(0, pic)
    assert lib.p264hip_copy_to_device(dev, bad.ctypes.data, n) == 0
    hip.input_commit(0)
    with pytest.raises(P264Error):
        hip.reconstruct([0], [0])
    dev, n = hip.input_reserve(0, pic)
    assert lib.p264hip_copy_to_device(dev, good.ctypes.data, n) == 0
    hip.input_commit(0)
    hip.reconstruct([0], [0])
    compare(hip.read_frame(0, DST), chk.reconstruct(pic), "the good picture behind the refused one", pic)
    # the host road says the same about the same record
    pic.rec["coef_mask"][m] = 0x7ff
    with pytest.raises(P264Error):
        hip.upload(1, [pic])
    hip.close()
