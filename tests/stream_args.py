"""Argument tables that more than one test module uses: stream-writer command lines, make_picture keywords and launch shapes.
Test ids are derived from their order and content.  Tables of one subject that has a helper module live there (slice_streams.py)."""
from tests import seam_fuzz

CIF = "--mbw 22 --mbh 18"


def cif(args):
    a = args.split()
    for k in ("--mbw", "--mbh"):
        i = a.index(k); del a[i:i + 2]
    return CIF + " " + " ".join(a)


# B pictures (tests/test_bslices.py)
B_STREAMS = [
    "--mbw 9 --mbh 7 --frames 22 --seed 81 --refs 2 --bframes 2 --coded 10 --maxlevel 6",
    "--mbw 8 --mbh 6 --frames 26 --seed 82 --refs 3 --bframes 3 --sub8x8 --implicit --coded 10 --maxlevel 6",
    "--mbw 8 --mbh 6 --frames 22 --seed 83 --refs 2 --bframes 2 --temporal --sub8x8 --coded 8 --maxlevel 6",
    "--mbw 7 --mbh 6 --frames 19 --seed 84 --refs 2 --bframes 1 --d8inf --sub8x8 --coded 8 --maxlevel 6",
    "--mbw 7 --mbh 5 --frames 25 --seed 85 --refs 4 --bframes 3 --temporal --d8inf --implicit --slices 2 --coded 8 --maxlevel 6",
]
# the CABAC / CAVLC twins (tests/test_cabac_streams.py)
CABAC_STREAMS = [
    "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 101 --coded 25 --maxlevel 40 --qp-delta 6",                      # I + P, large levels (escape codes)
    "--mbw 8 --mbh 6 --frames 10 --gop 0 --seed 102 --refs 2 --sub8x8 --slices 3 --coded 20 --maxlevel 12",     # two references, sub-8x8, slices
    "--mbw 11 --mbh 5 --frames 6 --intra-only --seed 103 --coded 45 --maxlevel 2000",                             # I only, dense, huge levels
    "--mbw 8 --mbh 6 --frames 16 --seed 104 --refs 2 --bframes 2 --sub8x8 --implicit --coded 12 --maxlevel 8",  # B, spatial direct
    "--mbw 7 --mbh 6 --frames 16 --seed 105 --refs 3 --bframes 3 --temporal --d8inf --slices 2 --coded 10 --maxlevel 8 --qp-delta 4",
    "--mbw 6 --mbh 5 --frames 8 --gop 0 --seed 106 --mvmax 600 --coded 8 --maxlevel 6",                          # long vectors: mvd escape codes
]
# the streams of the differential parse (each also with --cabac) and, CIF-sized, of tests/test_gpu_ipcm.py
IPCM_STREAMS = {
    "i_only": "--mbw 9 --mbh 7 --frames 4 --intra-only --seed 301 --coded 30 --ipcm 20",
    "ip_baseline": "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 302 --coded 25 --maxlevel 12 --ipcm 15",
    "b_spatial": "--mbw 8 --mbh 6 --frames 13 --seed 303 --refs 2 --bframes 2 --sub8x8 --implicit --coded 12 --maxlevel 8 --ipcm 12",
    "b_temporal": "--mbw 7 --mbh 6 --frames 13 --seed 304 --refs 3 --bframes 2 --temporal --d8inf --coded 10 --maxlevel 8 --ipcm 12",
    "refs2_sub8x8": "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 305 --refs 2 --sub8x8 --coded 20 --maxlevel 12 --ipcm 20",
    "qp_delta": "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 306 --qp 28 --qp-delta 6 --coded 35 --maxlevel 8 --ipcm 25",
    "slices3": "--mbw 8 --mbh 6 --frames 8 --gop 4 --seed 307 --slices 3 --coded 20 --maxlevel 12 --ipcm 40",
    "all_ipcm": "--mbw 6 --mbh 5 --frames 6 --gop 3 --seed 308 --slices 3 --ipcm 100",
    "style_flat": "--mbw 8 --mbh 6 --frames 6 --gop 3 --seed 309 --coded 20 --ipcm 30 --ipcm-style flat",
    "style_edge": "--mbw 8 --mbh 6 --frames 6 --gop 3 --seed 310 --coded 20 --ipcm 30 --ipcm-style edge",
}
# explicit weighted prediction (tests/test_weighted_pred_cpu.py)
WP_STREAMS = {
    "p_cavlc": "--mbw 6 --mbh 4 --frames 8 --gop 0 --seed 71 --refs 2 --wp --sub8x8 --slices 2 --coded 20 --maxlevel 8",
    "p_cabac": "--mbw 5 --mbh 3 --frames 6 --gop 0 --seed 72 --refs 2 --wp --cabac --coded 20 --maxlevel 8",
    "b_cabac": "--mbw 5 --mbh 4 --frames 9 --seed 73 --refs 2 --bframes 2 --wp --wp-bi --cabac --coded 20 --maxlevel 8",
    "b_cavlc_slices": "--mbw 6 --mbh 4 --frames 7 --seed 74 --refs 3 --bframes 2 --wp --wp-bi --slices 3 --coded 20 --maxlevel 8",
    "dup": "--mbw 6 --mbh 4 --frames 6 --gop 0 --seed 75 --refs 2 --wp --wp-dup --coded 20 --maxlevel 8",
}
# constrained intra prediction: every stream with CI appended
CI = " --constrained-intra --intra-pct 35"
CI_STREAMS = {
    "ip": "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 401 --coded 25 --maxlevel 12",
    "b": "--mbw 8 --mbh 6 --frames 13 --seed 402 --refs 2 --bframes 2 --sub8x8 --implicit --coded 12 --maxlevel 8",
    "slices3": "--mbw 8 --mbh 6 --frames 8 --gop 4 --seed 403 --slices 3 --coded 20 --maxlevel 12",
    "ipcm": "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 404 --coded 25 --maxlevel 12 --ipcm 15",
    "sub8x8": "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 405 --refs 2 --sub8x8 --coded 20 --maxlevel 12",
}
# several slices per picture (the reference handles one, decoder/decoder.c:516-523): slice boundaries in the middle of
# macroblock rows change every neighbour-availability pattern of the intra predictors and the vector / nC / mode predictors
SLICED = ["--mbw 11 --mbh 9 --frames 8 --gop 4 --seed 43 --slices 4 --coded 10 --maxlevel 6",
          "--mbw 7 --mbh 6 --frames 9 --gop 0 --seed 44 --slices 5 --refs 2 --coded 12 --maxlevel 6",
          "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 45 --slices 3 --deblock-idc 2 --coded 14 --maxlevel 8"]   # no filtering across slices
# sub-8x8 partitions (8x4, 4x8, 4x4; the reference mis-decodes them, A-Q4) and list-0 reordering (ignored by the reference,
# decoder/lists.c:146-149): spec-driven, pinned by the writer's record and by HIP == oracle
SUB8X8 = ["--mbw 11 --mbh 9 --frames 8 --gop 4 --seed 46 --sub8x8 --coded 10 --maxlevel 6",
          "--mbw 9 --mbh 8 --frames 9 --gop 0 --seed 47 --sub8x8 --refs 2 --slices 2 --mvmax 40 --coded 12 --maxlevel 6"]
REORDER = "--mbw 10 --mbh 8 --frames 12 --gop 0 --seed 48 --refs 2 --reorder --sub8x8 --coded 10 --maxlevel 6"
MMCO = ["--mbw 8 --mbh 6 --frames 40 --gop 14 --seed 71 --refs 3 --mmco --coded 8 --maxlevel 6",
        "--mbw 7 --mbh 5 --frames 36 --gop 0 --seed 72 --refs 4 --mmco --sub8x8 --coded 8 --maxlevel 6",
        # operation 5 too: everything but the current picture goes, which then counts as frame_num 0 (7.4.3, 8.2.1) - the
        # pictures behind it (at least num_ref_frames P pictures before the next one) build their lists against that
        "--mbw 7 --mbh 5 --frames 60 --gop 0 --seed 73 --refs 3 --mmco5 --coded 8 --maxlevel 6"]
# reference lists that grow to 16 entries in a store of 17 slots (tests/test_long_lists_streams_cpu.py): 7 x 5 macroblocks, more
# pictures than the window holds - a P stream more than 17 pictures, a B stream more than 17 reference pictures
LONG_LISTS_COMMON = "--mbw 7 --mbh 5 --coded 8 --maxlevel 6"
LONG_LISTS = {
    "p_cavlc": LONG_LISTS_COMMON + " --frames 24 --gop 0 --seed 161 --refs 16 --sub8x8",
    "p_cavlc_mmco": LONG_LISTS_COMMON + " --frames 44 --gop 0 --seed 162 --refs 16 --sub8x8 --mmco",
    "p_cabac_9": LONG_LISTS_COMMON + " --frames 16 --gop 0 --seed 163 --refs 9 --cabac",
    "b_cabac_temporal": LONG_LISTS_COMMON + " --frames 58 --seed 164 --refs 16 --bframes 2 --implicit --temporal --cabac",
    "b_cavlc_wp_8": LONG_LISTS_COMMON + " --frames 37 --seed 165 --refs 8 --bframes 2 --wp --wp-bi",
    "p_slice_lists_6": LONG_LISTS_COMMON + " --frames 12 --gop 0 --seed 166 --refs 6 --slices 3 --slice-lists",
}
B_CIF = "--mbw 22 --mbh 18 --frames 7 --seed 5 --refs 2 --bframes 2 --implicit --d8inf --coded 8 --maxlevel 8"      # I P B B P B B

LAUNCH_SHAPES = [  # (P264AMD_DEBLOCK_RB_LOG2, P264AMD_DEBLOCK_PICS_PER_WG, P264AMD_INTRA_WAVES)
    ("3", "1", "16"), ("2", "2", "8"), ("2", "1", "4"), ("1", "4", "8"), ("1", "3", "1"), ("1", "1", "16"),
    # more pictures per workgroup than a wavefront holds: groups (the last one partly empty with 7 streams)
    ("2", "4", "8"), ("3", "4", "8"), ("2", "7", "4"), ("3", "16", "4"), ("1", "13", "2"),
]
# the batches of tests/test_gpu_distinct_shapes.py, which tests/test_distinct_pool_cpu.py checks for workgroups with one source twice
DISTINCT_STREAMS = 37                    # more than two pools' worth, prime - the last workgroup of every shape is partly empty
ODD = ["3", "5", "7", "13"]                # odd pictures per k_deblock workgroup
# (P264AMD_DEBLOCK_RB_LOG2, P264AMD_DEBLOCK_PICS_PER_WG, P264AMD_DEBLOCK_WAVES): more units than wavefronts
WAVES = [("2", "4", "3"), ("3", "4", "5"), ("1", "8", "1"), ("2", "7", "2"), ("3", "3", "2")]

# tests/test_gpu_seam_fuzz.py and its CPU twin
SEAM_CONFIGS = [
    # name, mb_w, mb_h, pictures, make_picture keywords
    ("typical", 9, 7, 6, dict(level_style="small", qp_mode="random", n_ref=1, slots=2)),
    ("int16_wrap", 7, 5, 6, dict(level_style="wrap", qp_mode="random", n_ref=1, slots=2)),
    ("mixed_levels_3refs", 8, 6, 8, dict(level_style="mixed", qp_mode="random", n_ref=3, slots=4, slices=3)),
    ("two_qps_smooth", 10, 6, 6, dict(level_style="small", qp_mode="two", n_ref=2, slots=3, mv_range=12)),
    ("far_vectors", 6, 5, 5, dict(level_style="small", qp_mode=30, n_ref=1, slots=2, mv_range=600)),
    ("quadrant_partitions_only", 9, 6, 6, dict(level_style="large", qp_mode="random", n_ref=2, slots=3, sub8x8=False)),
    ("sliced_single_column", 1, 9, 5, dict(level_style="mixed", qp_mode="random", n_ref=1, slots=2, slices=4)),
    ("single_row", 11, 1, 5, dict(level_style="mixed", qp_mode="random", n_ref=1, slots=2, slices=3)),
    ("wide_picture", 67, 3, 4, dict(level_style="small", qp_mode="random", n_ref=2, slots=3)),
    # B pictures: two lists in the seam, every 8x8 quadrant from list 0, list 1 or both, plain and
    # implicit-weight averages (core/macroblock.c:525-583, core/mc.c:76-132).  The reference cannot decode B slices: these
    # are pinned to the oracle, whose two combines are pinned to the reference's function tables (kat_bipred.npz).
    ("b_pictures", 9, 7, 8, dict(level_style="small", qp_mode="random", n_ref=2, slots=4, b_picture=True, n_ref_l1=2)),
    ("b_pictures_far_wrap", 7, 6, 6, dict(level_style="mixed", qp_mode="random", n_ref=1, slots=3, b_picture=True, n_ref_l1=2, mv_range=500, slices=2)),
    ("b_pictures_weighted_smooth", 10, 6, 6, dict(level_style="small", qp_mode="two", n_ref=3, slots=4, b_picture=True, n_ref_l1=1, weighted=True, mv_range=12)),
    # the same two frames in both lists, in opposite order, and list-1 vectors that often repeat the list-0 vectors: neighbouring
    # blocks reach one picture through different lists (or crossed) with equal vectors - boundary strength 0 by H.264 8.7.2.1,
    # 1 by a list-by-list comparison of the indices (what core/frame.c:565-577 does)
    ("b_same_frames_swapped_lists", 10, 7, 8, dict(level_style="small", qp_mode="two", n_ref=2, slots=3, b_picture=True, n_ref_l1=2, mv_range=6, mirror_l1=0.7, sub8x8=False)),
]

# the kinds of picture a batch is composed of (tests/test_gpu_batch_composition.py, tests/test_gpu_ipcm_batch.py)
SLOTS, DST = 4, 3                # reference frames in slots 0 .. 2, every picture writes slot 3
KINDS = {
    "I": dict(p_picture=False),
    "P": dict(n_ref=1),
    "P_multi_dup": dict(n_ref=3, dup_refs=True),
    "P_weighted": dict(n_ref=2, explicit_wp="legal"),
    "B": dict(n_ref=2, n_ref_l1=2, b_picture=True, weighted=False),
    "B_implicit": dict(n_ref=2, n_ref_l1=2, b_picture=True, weighted=True),
    "B_weighted": dict(n_ref=2, n_ref_l1=2, b_picture=True, explicit_wp="legal"),
}
PLAIN_P = {"P"}                  # the kinds whose batches alone keep the fused edge-info pass (P_multi_dup: one frame at two indices -
                                 # the loop filter compares pictures, H.264 8.7.2.1, which the two-list edge-info kernel does)


def draw(rng, mb_w, mb_h, kind):
    return seam_fuzz.make_picture(rng, mb_w, mb_h, slots=SLOTS, dst_slot=DST, level_style="mixed", qp_mode="random", intra_share=0.2,
                                  slices=2, **KINDS[kind])
