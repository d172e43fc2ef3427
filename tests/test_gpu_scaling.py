"""Scaling matrices on the MI355X: the pictures of tests/scaling_stim.py (weights over the whole byte: 0, 1 .. 3, 4 .. 64 and
65 .. 255 - extreme_set) through p264hip_submit, in batches of three through the
upload, compact and commit roads, and in one batch that mixes scaled and flat pictures of every kind, all three planes byte for byte
against tests/scaling_checker.py (H.264 8.5.9 - 8.5.13 with the picture's lists: the reference forces flat lists and is no oracle
here); what the launch reports; all-16 lists against the flat decode of the same pictures; two whole streams whose parameter sets
carry matrices through the parser, the drop-in decoder and the command-line decoder."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import hip_harness as H
from tests import i8x8_stim as IS
from tests import residual_checker as RC
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import seam_fuzz
from tests import synth_cases

pytestmark = pytest.mark.gpu
SLOTS = 3


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    return {which: [(st, H.expect(st, SC.SpecRecon, SLOTS)) for st in getattr(SS, which)()] for which in SS.SETS}


def scaled_in(hip, batch):
    return hip.last_scaled_pictures(), sum(bool(int(st.pic.desc.scaling_lists)) for st, _ in batch)


@pytest.mark.parametrize("which", SS.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    def probe(hip, st):
        assert hip.last_scaled_pictures() == 1 and hip.last_t8x8_wgs() == 0
    bad, sent = H.submit_each(lib, expected[which], SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    SS.assert_covered(which, sent)


@pytest.mark.parametrize("road", ["upload", "compact", "commit"])
def test_batches_of_three_equal_the_standard(lib, expected, road):
    sent_all = []
    for size, cases in H.by_size(expected["directed_set"] + expected["random_set"] + expected["extreme_set"]).items():
        bad, sent, counts = H.run_batches(lib, cases, road=road, slots=SLOTS, probe=scaled_in)
        assert not bad, "%s: %d of %d pictures differ: %s" % (size, len(bad), len(sent), bad[:3])
        assert all(got == want == 3 for got, want in counts)
        sent_all += sent
    directed = {id(st.pic) for st, _ in expected["directed_set"]}
    SS.assert_covered("directed_set", [st for st in {id(st.pic): st for st in sent_all}.values() if id(st.pic) in directed])
    extreme = {id(st.pic) for st, _ in expected["extreme_set"]}
    SS.assert_covered("extreme_set", [st for st in {id(st.pic): st for st in sent_all}.values() if id(st.pic) in extreme])


def flat_cases():
    """flat pictures of 6 x 5: P, P with T8X8 and Intra 8x8 records, Intra 8x8 without T8X8, B"""
    rng = np.random.default_rng(8595)
    plain = seam_fuzz.make_picture(rng, IS.MB_W, IS.MB_H, n_ref=2, slots=3, dst_slot=0, level_style="small", qp_mode="random", intra_share=0.1)
    RC.make_conformant(plain)
    i8 = IS.inter_set(seed=8596)
    out = [IS.Stim("flat P", plain, SS.S.frames_for(rng, IS.MB_W, IS.MB_H), 0, 0), i8[0], i8[1], i8[4]]
    assert not any(int(st.pic.desc.scaling_lists) for st in out)
    return [(st, H.expect(st, SC.SpecRecon, SLOTS)) for st in out]


def test_a_mixed_batch_and_what_the_launch_reports(lib, expected):
    """scaled P, scaled B, scaled explicit-weight and scaled I pictures beside flat P, flat T8X8 and flat Intra 8x8 pictures in ONE batch:
    every picture as the standard says - the flat ones what the flat kernels write; a flat-only batch reports 0 and decodes as ever"""
    d = {st.name: (st, want) for st, want in expected["directed_set"]}
    flat = flat_cases()
    mixed = [d["I8X8 P cluster"], flat[0], d["I8X8 B cluster"], flat[1], d["I8X8 P cluster weighted"], flat[2], d["scaled I picture 0"], flat[3]]
    kinds = {(int(st.pic.desc.slice_type), bool(st.pic.desc.explicit_wp), bool(int(st.pic.desc.scaling_lists))) for st, _ in mixed}
    assert kinds >= {(N.SLICE_P, False, True), (N.SLICE_B, False, True), (N.SLICE_P, True, True), (N.SLICE_I, False, True), (N.SLICE_P, False, False), (N.SLICE_B, False, False)}
    rec = lambda st: st.pic.mb_records()["intra_modes"]
    assert any((rec(st) & N.MB_T8X8).any() for st, _ in flat) and any((rec(st) & N.MB_I8X8).any() and not (rec(st) & N.MB_T8X8).any() for st, _ in flat)
    bad, sent, counts = H.run_batches(lib, mixed, n=len(mixed), slots=SLOTS, probe=scaled_in)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert counts == [(4, 4)]
    # without the I picture: the sparse intra instance
    bad, sent, counts = H.run_batches(lib, mixed[:6], n=6, slots=SLOTS, probe=scaled_in)
    assert not bad and counts == [(3, 3)], bad[:3]
    # flat only
    def probe(hip, batch):
        return hip.last_scaled_pictures(), hip.last_t8x8_wgs() > 0, hip.last_intra_i8()
    bad, sent, seen = H.run_batches(lib, flat, n=len(flat), slots=SLOTS, probe=probe)
    assert not bad and seen == [(0, True, 1)], (bad[:3], seen)


def test_all_16_lists_equal_the_flat_decode(lib):
    """scaling_lists = 1 with every weight 16 goes through the scaled kernels and gives, byte for byte, what the flat kernels give for
    the same (conformant) picture with scaling_lists = 0"""
    for a, b in SS.flat_twins():
        want = H.expect(b, SC.SpecRecon, SLOTS)
        with H.reconstructor(lib, a.pic.mb_w, a.pic.mb_h, n_streams=2, slots=SLOTS, max_pictures=2) as hip:
            for k, st in enumerate((a, b)):
                H.load_frames(hip, k, st.frames)
            hip.upload(0, [a.pic])
            hip.reconstruct([0], [0])
            assert hip.last_scaled_pictures() == 1
            hip.upload(1, [b.pic])
            hip.reconstruct([1], [1])
            assert hip.last_scaled_pictures() == 0
            got_a, got_b = hip.read_frame(0, a.pic.desc.dst_slot), hip.read_frame(1, b.pic.desc.dst_slot)
        H.compare(got_b, want, b.name, b.pic)
        H.compare(got_a, got_b, a.name + " against the flat kernels", a.pic)


# ---- whole streams -------------------------------------------------------------------------------------------------------------
# --qp / --maxlevel / --coded: the t8x8 stream's (tests/test_gpu_t8x8.py: 14 / 3 / 35); JVT weights reach 42 and stay in range with them, the
# random lists reach 64 and need --maxlevel 2.  The test asserts that the checker's range census is clean on every picture: no
# macroblock is left out of the comparison.
STREAMS = {
    "cabac b jvt sps": "--mbw 8 --mbh 6 --frames 10 --refs 2 --bframes 2 --d8inf --cabac --t8x8 70 --i8x8 50 --qp 14 --qp-delta 3 --coded 35 --maxlevel 3 --seed 86 --cqm jvt --cqm-where sps",
    "cavlc p rand both": "--mbw 8 --mbh 6 --frames 10 --refs 2 --t8x8 70 --i8x8 50 --qp 14 --qp-delta 3 --coded 35 --maxlevel 2 --seed 87 --cqm rand:7 --cqm-where both",
}


@pytest.mark.parametrize("which", list(STREAMS))
def test_a_stream_with_scaling_matrices_end_to_end(lib, tmp_path, which):
    """synth264 --cqm (High profile, 8x8 transform in inter and intra macroblocks) through the parser and p264hip_submit, through the
    drop-in decoder and through the command-line decoder: every picture equals the standard's with the stream's lists"""
    data = open(synth_cases.generate(STREAMS[which]), "rb").read()
    pics, slots, want, spec = H.parse_and_expect(lib, data, SC.SpecRecon, intra8x8=True, scaling=True)
    assert len(pics) == 10 and all(int(p.desc.scaling_lists) == 1 for p in pics) and spec.scaled == 10
    types = {int(p.desc.slice_type) for p in pics}
    assert types == ({N.SLICE_I, N.SLICE_P, N.SLICE_B} if "--bframes" in STREAMS[which] else {N.SLICE_I, N.SLICE_P})
    for i, p in enumerate(pics):
        n, out = SC.census(p)
        assert n and not out, "picture %d: %d level blocks feed a value out of range: %s" % (i, len(out), sorted(out)[:3])
    t8 = sum(int(((p.mb_records()["intra_modes"] & N.MB_T8X8) != 0).sum()) for p in pics)
    i8 = sum(int(((p.mb_records()["intra_modes"] & N.MB_I8X8) != 0).sum()) for p in pics)
    assert t8 >= 60 and i8 >= 10 and spec.met >= 3, (t8, i8, spec.met)
    seen = SS.survey([SS.Stim("picture %d" % i, p, {}, 0) for i, p in enumerate(pics)])
    assert all(seen.lists[n] > 0 for n in range(8)), dict(seen.lists)
    table = bytes(pics[0].desc.scaling4x4) + bytes(pics[0].desc.scaling8x8)
    assert (table == SC.table_bytes(SC.DEFAULTS)) == ("jvt" in which) and all(bytes(p.desc.scaling4x4) + bytes(p.desc.scaling8x8) == table for p in pics)

    def probe(hip, i, p):
        assert hip.last_scaled_pictures() == 1
    H.submit_stream(lib, pics, slots, want, "p264hip_submit", probe)
    got = H.dropin_pictures(lib, data)
    assert len(got) == 10
    H.compare_pictures(got, want, "drop-in decoder", crop=True)
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want), "the command-line decoder's pictures differ from the standard's"
