"""The configurations of tests/test_gpu_wp_seam_fuzz.py and its CPU twins, and their inputs drawn from each configuration's seed."""
import numpy as np

from tests import seam_fuzz

CONFIGS = [
    # name, mb_w, mb_h, pictures, make_picture keywords.  Picture 2 is an I picture (the store moves on, no table).
    ("p_sub4x4_3refs_dup", 8, 6, 6, dict(n_ref=3, slots=3, level_style="wrap", qp_mode="random", intra_share=0.3, slices=3,
                                          slice_idcs=[0, 1, 2], explicit_wp="legal")),
    ("b_sub8x8_legal", 9, 7, 6, dict(n_ref=2, n_ref_l1=2, slots=4, b_picture=True, level_style="small", qp_mode="random", explicit_wp="legal")),
    ("b_wide_smooth", 10, 6, 6, dict(n_ref=2, n_ref_l1=2, slots=4, b_picture=True, level_style="small", qp_mode="two", mv_range=12, explicit_wp="wide")),
    ("p_far", 6, 5, 5, dict(n_ref=2, slots=3, level_style="small", qp_mode=30, mv_range=500, explicit_wp="legal")),
    ("b_far", 7, 6, 5, dict(n_ref=2, n_ref_l1=2, slots=4, b_picture=True, level_style="mixed", qp_mode="random", mv_range=500, slices=2, explicit_wp="legal")),
    ("b_dup_lists", 8, 6, 5, dict(n_ref=3, n_ref_l1=3, slots=4, b_picture=True, level_style="small", qp_mode="random", dup_refs=True, explicit_wp="legal")),
    ("p_single_column", 1, 9, 5, dict(n_ref=2, slots=3, level_style="mixed", qp_mode="random", slices=4, explicit_wp="legal")),
    ("b_single_row", 11, 1, 5, dict(n_ref=2, n_ref_l1=2, slots=4, b_picture=True, level_style="mixed", qp_mode="random", slices=3, explicit_wp="wide")),
    ("b_wide_picture", 67, 3, 5, dict(n_ref=2, n_ref_l1=2, slots=4, b_picture=True, level_style="small", qp_mode="random", explicit_wp="legal")),
    # indices n_ref .. 15 in both lists: entry 0 for the prediction, both kinds of weights and the loop filter
    ("past_list_p", 8, 6, 5, dict(n_ref=2, slots=4, level_style="small", qp_mode="random", mv_range=12, past_list=0.3)),
    ("past_list_b", 8, 6, 5, dict(n_ref=3, n_ref_l1=2, slots=4, b_picture=True, level_style="small", qp_mode="random", mv_range=12, past_list=0.3)),
    ("past_list_wp_p", 8, 6, 5, dict(n_ref=3, slots=4, level_style="small", qp_mode="random", mv_range=12, past_list=0.3, explicit_wp="legal")),
    ("past_list_wp_b", 8, 6, 5, dict(n_ref=3, n_ref_l1=2, slots=4, b_picture=True, level_style="small", qp_mode="random", mv_range=12, past_list=0.3, explicit_wp="legal")),
]
FORCED_DENOMS = {0: (0, 7), 1: (7, 0)}       # picture -> (luma, chroma): both ends of the denominator in every config


def config_inputs(name, mb_w, mb_h, n_pics, kw):
    """a config's starting frames (one per store slot), then its pictures - drawn lazily, in this order, from the config's seed"""
    rng = np.random.default_rng(sum(map(ord, name)) * 7727)
    kind = "smooth" if ("smooth" in name or "past_list" in name) else "noise"
    yield [seam_fuzz.random_frame(rng, mb_w, mb_h, kind) for _ in range(kw["slots"])]
    for i in range(n_pics):
        yield seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=(i != 2), dst_slot=i % kw["slots"], wp_denoms=FORCED_DENOMS.get(i), **kw)
