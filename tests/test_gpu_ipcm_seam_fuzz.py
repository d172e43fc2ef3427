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
from tests.hip_harness import ROADS, compare, put, reconstructor
from tests.ipcm_seam_stim import CONFIGS, DST, S, SLOTS, check_coverage, prepare


@pytest.mark.gpu
@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_ipcm_seam_fuzz(lib, oracle, name, with_i):
    mb_w, mb_h, share, samples, kw = CONFIGS[name]
    batch, seen = prepare(oracle, name, with_i)
    with reconstructor(lib, mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S) as hip:
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
    check_coverage(name, with_i, seen)


def test_coverage_of_the_drawn_batches(oracle):
    """(CPU) the same figures without a device"""
    for name in CONFIGS:
        for with_i in (False, True):
            check_coverage(name, with_i, prepare(oracle, name, with_i)[1])


@pytest.mark.gpu
def test_ipcm_1080p_batch(lib, oracle):
    rng = np.random.default_rng(1080)
    mb_w, mb_h = 120, 68
    with reconstructor(lib, mb_w, mb_h, n_streams=S, slots=SLOTS, max_pictures=S) as hip:
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


@pytest.mark.gpu
def test_a_committed_ipcm_record_with_a_short_mask_is_refused(lib, oracle):
    """mask 0x7ff on an I_PCM record in the middle of the picture (more than twelve blocks of coefs[] behind its coef_index: even a
    kernel that ran it unchecked would read inside the slot): p264hip_reconstruct says P264HIP_EINVAL, and the context decodes a
    good picture right afterwards"""
    rng = np.random.default_rng(4242)
    mb_w, mb_h = 9, 7
    chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, SLOTS)
    with reconstructor(lib, mb_w, mb_h, n_streams=1, slots=SLOTS, max_pictures=2) as hip:
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
