"""tests/intra_checker.py checks itself (CPU): a table of hand-computed predictions a reader can hold against H.264 8.3 without
running anything else; byte equality with the oracle on single-slice pictures of every kind (where the reference's DC fall-back
keyed on the top-left flag, SURVEY A-Q7, and the standard's keyed on left and top coincide - this ties the checker to the
reference through the hashes that pin the oracle on those streams); and byte equality on multi-slice pictures, where the two
rules differ for the macroblock below a slice's first macroblock.  On the parent of the commit that brought this file the oracle predicted DC_LEFT there, and seven of the ten multi-slice cases
fail: the SLICED streams with 3395 / 5315 / 2285 differing samples (the first in picture 4, plane 1, (y=55, x=67) - the chroma row
the loop filter changes above such a macroblock; picture 0, plane 0, (y=46, x=32); picture 4, plane 1, (y=39, x=57)), the weighted
three-slice B stream with 720 (picture 0, plane 2, (y=15, x=16)), the seam fuzz with 2, 3, 4 slices with 45 / 2819 / 353; the
I_PCM three-slice stream, the two-slice B stream and the CABAC two-slice B stream hold no such macroblock with a DC mode."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import intra_checker as ic
from tests import pcm_checker, pcm_fuzz, seam_fuzz, synth_cases
from tests.hip_harness import decode_both, differences
from tests.stream_args import B_STREAMS, CABAC_STREAMS, IPCM_STREAMS, SLICED, WP_STREAMS
from tests.synth_cases import write_stream as synth

L4, T4, TR4, C4 = [10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120], 45
T8 = T4 + TR4
T8_REPLICATED = [50, 60, 70, 80, 80, 80, 80, 80]
L16, T16 = list(range(10, 26)), list(range(100, 116))            # sums 280 and 1720
RAMP16 = [102 + 2 * x for x in range(16)]                        # p[x, -1] = 100 + 2 (x + 1): the corner continues it with 100
LC, TC = [10, 11, 12, 13, 50, 51, 52, 53], [100, 101, 102, 103, 200, 201, 202, 203]   # half sums 46, 206 and 406, 806
RAMP8 = RAMP16[:8]


def blocks(a, b, c, d):
    """an 8x8 of four flat 4x4 blocks: a b / c d"""
    return [[a] * 4 + [b] * 4] * 4 + [[c] * 4 + [d] * 4] * 4


# (what, predictor, mode, left, top, corner, expected [y][x])
TABLE = [
    # 8.3.1.2.3: (sum of 8 + 4) >> 3 = 364 >> 3; one side (sum of 4 + 2) >> 2 = 102 >> 2 and 262 >> 2; none 128
    ("4x4 DC, left and top", ic.pred4x4, 2, L4, T8, C4, [[45] * 4] * 4),
    ("4x4 DC, left only", ic.pred4x4, 2, L4, None, None, [[25] * 4] * 4),
    ("4x4 DC, top only", ic.pred4x4, 2, None, T8, None, [[65] * 4] * 4),
    ("4x4 DC, neither", ic.pred4x4, 2, None, None, None, [[128] * 4] * 4),
    # 8.3.1.2.4: on a ramp of step 10 the 1-2-1 filter returns the middle sample; (3, 3) is (110 + 3 * 120 + 2) >> 2
    ("4x4 down-left, top-right there", ic.pred4x4, 3, None, T8, None, [[60, 70, 80, 90], [70, 80, 90, 100], [80, 90, 100, 110], [90, 100, 110, 118]]),
    # ... with p[4..7, -1] = p[3, -1] = 80: (70 + 2 * 80 + 80 + 2) >> 2 = 78
    ("4x4 down-left, top-right replicated", ic.pred4x4, 3, None, T8_REPLICATED, None, [[60, 70, 78, 80], [70, 78, 80, 80], [78, 80, 80, 80], [80, 80, 80, 80]]),
    # 8.3.1.2.8: even rows (a + b + 1) >> 1, odd rows 1-2-1
    ("4x4 vertical-left, top-right replicated", ic.pred4x4, 7, None, T8_REPLICATED, None, [[55, 65, 75, 80], [60, 70, 78, 80], [65, 75, 80, 80], [70, 78, 80, 80]]),
    # 8.3.1.2.5: diagonal (50 + 2 * 45 + 10 + 2) >> 2 = 38; above it (45 + 100 + 60 + 2) >> 2 = 51, 60, 70; below it (45 + 20 + 20 + 2) >> 2 = 21,
    # (10 + 40 + 30 + 2) >> 2 = 20, (20 + 60 + 40 + 2) >> 2 = 30
    ("4x4 down-right", ic.pred4x4, 4, L4, T8, C4, [[38, 51, 60, 70], [21, 38, 51, 60], [20, 21, 38, 51], [30, 20, 21, 38]]),
    # 8.3.1.2.9: zHU = x + 2 y -> 15 20 25 30 35, zHU 5: (30 + 3 * 40 + 2) >> 2 = 38, beyond: p[-1, 3]
    ("4x4 horizontal-up", ic.pred4x4, 8, L4, None, None, [[15, 20, 25, 30], [25, 30, 35, 38], [35, 38, 40, 40], [40, 40, 40, 40]]),
    # 8.3.3.3: (2000 + 16) >> 5, (280 + 8) >> 4, (1720 + 8) >> 4, 128
    ("16x16 DC, left and top", ic.pred16x16, 2, L16, T16, None, [[63] * 16] * 16),
    ("16x16 DC, left only", ic.pred16x16, 2, L16, None, None, [[18] * 16] * 16),
    ("16x16 DC, top only", ic.pred16x16, 2, None, T16, 7, [[108] * 16] * 16),
    ("16x16 DC, neither", ic.pred16x16, 2, None, None, None, [[128] * 16] * 16),
    # 8.3.3.4: H = sum (i + 1) * 4 (i + 1) = 816, b = (5 * 816 + 32) >> 6 = 64, V = 0, c = 0, a = 16 * (100 + 132):
    # (3712 + 64 (x - 7) + 16) >> 5 = 102 + 2 x
    ("16x16 plane", ic.pred16x16, 3, [100] * 16, RAMP16, 100, [RAMP16] * 16),
    # 8.3.4.1-3: block (0, 0) (406 + 46 + 4) >> 3; (4, 0) top alone (806 + 2) >> 2; (0, 4) left alone (206 + 2) >> 2; (4, 4) (806 + 206 + 4) >> 3
    ("chroma DC, left and top", ic.pred_chroma, 0, LC, TC, None, blocks(57, 202, 52, 127)),
    # left only: (4, 0) has no top and takes ITS left samples, rows 0..3: (46 + 2) >> 2
    ("chroma DC, left only", ic.pred_chroma, 0, LC, None, None, blocks(12, 12, 52, 52)),
    # top only: (0, 4) has no left and takes ITS top samples, columns 0..3: (406 + 2) >> 2
    ("chroma DC, top only", ic.pred_chroma, 0, None, TC, 9, blocks(102, 202, 102, 202)),
    ("chroma DC, neither", ic.pred_chroma, 0, None, None, None, blocks(128, 128, 128, 128)),
    # 8.3.4.4: H = 4 * 30 = 120, b = (34 * 120 + 32) >> 6 = 64, c = 0, a = 16 * (100 + 116): (3456 + 64 (x - 3) + 16) >> 5 = 102 + 2 x
    ("chroma plane", ic.pred_chroma, 3, [100] * 8, RAMP8, 100, [RAMP8] * 8),
    ("chroma horizontal", ic.pred_chroma, 1, LC, None, None, [[v] * 8 for v in LC]),
    ("chroma vertical", ic.pred_chroma, 2, None, TC, None, [TC] * 8),
]


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_predictors_against_hand_computed_samples(case):
    what, fn, mode, left, top, corner, want = case
    assert fn(mode, left, top, corner).tolist() == want


def test_top_right_replication_and_block_availability():
    assert ic.top_with_topright(T4, TR4) == T8
    assert ic.top_with_topright(T4, None) == T8_REPLICATED           # 8.3.1.2: p[3, -1] for p[4..7, -1]
    assert ic.top_with_topright(None, TR4) is None
    for flags in range(16):
        L, T, TR, TL = bool(flags & 1), bool(flags & 2), bool(flags & 4), bool(flags & 8)
        av = [ic.block_availability(i, L, T, TR, TL) for i in range(16)]
        # top-right: the first row of blocks reads the macroblock above (the last one the macroblock above and to the right);
        # below it, blocks 3, 7, 11, 13, 15 look at a block that is decoded later or lies outside the macroblock
        assert [a[2] for a in av] == [T, T, True, False, T, TR, True, False, True, True, True, False, True, False, True, False]
        assert [a[0] for a in av] == [L, True, L, True, True, True, True, True, L, True, L, True, True, True, True, True]
        assert [a[1] for a in av] == [T, T, True, True, T, T, True, True] + [True] * 8
        assert [a[3] for a in av] == [TL, T, L, True, T, T, True, True, L, True, L, True, True, True, True, True]


@pytest.mark.parametrize("what,fn,mode,left,top,corner", [
    ("4x4 vertical without top", ic.pred4x4, 0, L4, None, C4), ("4x4 horizontal without left", ic.pred4x4, 1, None, T8, C4),
    ("4x4 down-left without top", ic.pred4x4, 3, L4, None, C4), ("4x4 down-right without corner", ic.pred4x4, 4, L4, T8, None),
    ("4x4 vertical-right without corner", ic.pred4x4, 5, L4, T8, None), ("4x4 horizontal-down without corner", ic.pred4x4, 6, L4, T8, None),
    ("4x4 horizontal-down without left", ic.pred4x4, 6, None, T8, C4), ("4x4 vertical-left without top", ic.pred4x4, 7, L4, None, C4),
    ("4x4 horizontal-up without left", ic.pred4x4, 8, None, T8, C4),
    ("16x16 vertical without top", ic.pred16x16, 0, L16, None, 1), ("16x16 horizontal without left", ic.pred16x16, 1, None, T16, 1),
    ("16x16 plane without corner", ic.pred16x16, 3, L16, T16, None), ("16x16 plane without left", ic.pred16x16, 3, None, T16, 1),
    ("chroma horizontal without left", ic.pred_chroma, 1, None, TC, 1), ("chroma vertical without top", ic.pred_chroma, 2, LC, None, 1),
    ("chroma plane without corner", ic.pred_chroma, 3, LC, TC, None), ("chroma plane without top", ic.pred_chroma, 3, LC, None, 1),
])
def test_a_mode_that_needs_a_missing_neighbour_is_an_error(what, fn, mode, left, top, corner):
    with pytest.raises(ValueError, match="not available"):
        fn(mode, left, top, corner)


# ---- against the oracle on streams ------------------------------------------------------------------------------------------
def n_intra(pics):
    return sum(int((p.mb_records()["mb_type"] <= N.MB_I16x16).sum()) for p in pics)


def test_f26_equals_the_oracle(oracle, lib, f26):
    pics, n, first, _ = decode_both(oracle, lib, f26, limit=12)
    assert len(pics) == 12 and pics[0].desc.slice_type == N.SLICE_I and sum(p.desc.slice_type == N.SLICE_P for p in pics) >= 10
    assert n == 0, first


@pytest.mark.parametrize("name,limit", [("cfg2_720p_intra", 2), ("cif_ip", None)])
def test_synthetic_single_slice_streams_equal_the_oracle(oracle, lib, name, limit):
    pics, n, first, _ = decode_both(oracle, lib, synth_cases.stream_bytes(name), limit=limit)
    assert len(pics) >= 2 and n_intra(pics) > 500
    assert n == 0, first


@pytest.mark.parametrize("what,args", [
    ("main_cabac_b", CABAC_STREAMS[3] + " --cabac"), ("ipcm", IPCM_STREAMS["ip_baseline"]), ("ipcm_b", IPCM_STREAMS["b_spatial"]),
    ("weighted_p", "--mbw 9 --mbh 7 --frames 8 --gop 4 --seed 72 --refs 2 --wp --cabac --coded 20 --maxlevel 8"),
    ("weighted_b", "--mbw 9 --mbh 7 --frames 9 --seed 73 --refs 2 --bframes 2 --wp --wp-bi --coded 20 --maxlevel 8")],
    ids=["main_cabac_b", "ipcm", "ipcm_b", "weighted_p", "weighted_b"])
def test_single_slice_b_ipcm_and_weighted_streams_equal_the_oracle(oracle, lib, tmp_path, what, args):
    assert "--slices" not in args
    pics, n, first, _ = decode_both(oracle, lib, synth(tmp_path, args))
    assert n_intra(pics) > 50
    if "b" in what.split("_"):
        assert any(p.desc.slice_type == N.SLICE_B and n_intra([p]) for p in pics), "no B picture with an intra macroblock"
    if "ipcm" in what:
        assert sum(len(p.ipcm_macroblocks()) for p in pics) > 20
    if "weighted" in what:
        assert any(p.desc.explicit_wp and n_intra([p]) for p in pics)
    assert n == 0, first


MULTI_SLICE = [("sliced%d" % i, a) for i, a in enumerate(SLICED)] + [("ipcm_slices3", IPCM_STREAMS["slices3"]), ("b_two_slices", B_STREAMS[4]),
                                                                    ("cabac_b_slices2", CABAC_STREAMS[4] + " --cabac"), ("weighted_b_slices3", WP_STREAMS["b_cavlc_slices"])]


@pytest.mark.parametrize("what,args", MULTI_SLICE, ids=[m[0] for m in MULTI_SLICE])
def test_multi_slice_streams_equal_the_oracle(oracle, lib, tmp_path, what, args):
    """several slices per picture: macroblocks with LEFT and TOP and without TOPLEFT predict Intra16x16 DC / chroma DC from both
    neighbours (8.3.3.3, 8.3.4)"""
    pics, n, first, chk = decode_both(oracle, lib, synth(tmp_path, args))
    if what.startswith("sliced") or what == "weighted_b_slices3":
        assert len(chk.dc_log) > 0, "no macroblock with LEFT and TOP and without TOPLEFT predicts DC"
    assert n == 0, first


@pytest.mark.parametrize("slices", [2, 3, 4])
def test_multi_slice_seam_fuzz_equals_the_oracle(oracle, slices):
    rng = np.random.default_rng(9000 + slices)
    mb_w, mb_h, slots = 8, 6, 3
    bad, quirk = [], 0
    for k in range(12):
        chk = ic.IntraChecker(oracle, mb_w, mb_h, slots)
        ref = pcm_checker.PcmChecker(oracle, mb_w, mb_h, slots)
        for s in range(slots):
            f = seam_fuzz.random_frame(rng, mb_w, mb_h)
            for a, b, c in zip(chk.store[s], ref.store[s], f):
                a[:] = c; b[:] = c
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=k % 4 != 3, b_picture=k % 4 == 1, slices=slices, intra_share=0.3, n_ref=2, n_ref_l1=2,
                                     slots=slots, dst_slot=2, level_style="mixed")
        if k % 3 == 2:
            pcm_fuzz.to_ipcm(rng, pic, 0.15)
        bad += differences(chk.reconstruct(pic), ref.reconstruct(pic), "picture %d" % k, pic)
        quirk += len(chk.dc_log)
    assert quirk > 0, "no macroblock with LEFT and TOP and without TOPLEFT predicts DC"
    assert not bad, "%d pictures differ, first: %s" % (len(bad), bad[0])
