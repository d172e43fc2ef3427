"""A picture with I_PCM macroblocks in every batch composition (in the manner of tests/test_gpu_batch_composition.py): alone,
paired with each of the seven existing kinds of picture, and all eight in one call - p264hip_reconstruct picks its kernels by the
whole batch (k_intra or k_intra_sparse, with or without the fused edge info, the B and weighted instances), and every picture
must be its checker frame every time."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import pcm_checker, pcm_fuzz, seam_fuzz
from tests.stream_args import DST, KINDS, PLAIN_P, SLOTS, draw
from tests.hip_harness import compare, reconstructor

pytestmark = pytest.mark.gpu


def test_an_ipcm_picture_alone_in_pairs_and_with_everything(lib, oracle):
    rng = np.random.default_rng(2025)
    mb_w, mb_h = 6, 5
    kinds = ["P_ipcm"] + list(KINDS)
    with reconstructor(lib, mb_w, mb_h, n_streams=len(kinds), slots=SLOTS, max_pictures=len(kinds)) as hip:
        pics, want = [], []
        for s, kind in enumerate(kinds):
            chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, SLOTS)
            for slot in range(DST):
                f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if (s + slot) % 2 else "noise")
                for dst, src in zip(chk.store[slot], f):
                    dst[:] = src
                hip.write_frame(s, slot, *f)
            pic = draw(rng, mb_w, mb_h, "P" if s == 0 else kind)
            if s == 0:
                pcm_fuzz.to_ipcm(rng, pic, 0.35)
                assert (pic.rec["mb_type"] == N.MB_IPCM).sum() >= 5
            pics.append(pic)
            want.append([a.copy() for a in chk.reconstruct(pic)])
        blank = [np.zeros_like(a) for a in want[0]]
        for members in [(0,)] + [(0, s) for s in range(1, len(kinds))] + [(s, 0) for s in (1, 5)] + [tuple(range(len(kinds)))]:
            for s in members:
                hip.write_frame(s, DST, *blank)
            hip.upload(0, [pics[s] for s in members])
            hip.reconstruct(list(range(len(members))), list(members))
            li = hip.last_launch()
            names = [kinds[s] for s in members]
            assert (li["edge_info_fused"] > 0) == ({k for k in names if k != "P_ipcm"} <= PLAIN_P), (names, li)
            for s in members:
                compare(hip.read_frame(s, DST), want[s], "%s in batch %s" % (kinds[s], names), pics[s])
