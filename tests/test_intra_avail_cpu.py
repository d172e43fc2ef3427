"""The CPU twin of tests/test_gpu_intra_avail.py: the same drawn batches through the oracle (with pcm_checker's composition for
I_PCM and explicit weights) and through the intra checker, bytes of all three planes; the same coverage assertions; and the
seam fuzz's default mode still draws, seed for seed, the pictures it drew before it learnt the free mode."""
import numpy as np
import pytest

from tests import pcm_checker, seam_fuzz
from tests import intra_avail_stim as G
from tests.hip_harness import first_difference


@pytest.mark.parametrize("with_i", [False, True], ids=["p_b_only", "with_i_picture"])
@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_oracle_equals_the_intra_checker(oracle, name, with_i):
    mb_w, mb_h = G.FAMILIES[name][:2]
    batch, log = G.prepare(oracle, name, with_i)
    for s, (pic, f, want) in enumerate(batch):
        ref = pcm_checker.PcmChecker(oracle, mb_w, mb_h, G.SLOTS)
        for slot in range(G.DST):
            for dst, src in zip(ref.store[slot], f):
                dst[:] = src
        d = first_difference(ref.reconstruct(pic), want, "%s stream %d" % (name, s), pic)
        assert d is None, d
    if "directed" in name:
        G.check_directed(name, with_i, batch, log)


def test_coverage_of_the_drawn_batches():
    G.check_coverage(G.survey_all())


def test_default_mode_draws_what_it_drew_before_the_free_mode():
    """digests of pictures drawn by the builder as it was before avail_mode, slice_starts and force existed"""
    cases = [
        (0, 8, 6, dict(slices=3, intra_share=0.3, n_ref=2, slots=3), "12175b013be0aea4"),
        (1, 9, 7, dict(p_picture=False, level_style="mixed"), "0f7b92fd8f6817d9"),
        (2, 7, 5, dict(b_picture=True, n_ref=2, n_ref_l1=2, slots=4, slices=2, explicit_wp="legal"), "f362ddd6a587a8e5"),
        (3, 67, 3, dict(n_ref=2, slots=3, past_list=0.2, qp_mode="two"), "e86a882849989364"),
        (4, 1, 9, dict(slices=4, level_style="wrap"), "c2fd266a207b2556"),
    ]
    for seed, w, h, kw, want in cases:
        assert seam_fuzz.picture_digest(seam_fuzz.make_picture(np.random.default_rng(seed), w, h, **kw)) == want, "seed %d" % seed
    free = seam_fuzz.make_picture(np.random.default_rng(0), 8, 6, avail_mode="free", **cases[0][3])
    assert seam_fuzz.picture_digest(free) != cases[0][4]
