"""The 8x8 transform of inter macroblocks on the MI355X: the pictures of tests/t8x8_stim.py through p264hip_submit, through
p264hip_upload + p264hip_reconstruct in batches of three and through the compact road, all three planes byte for byte against
tests/t8x8_checker.py (H.264 8.5.6, 8.5.9, 8.5.13, 8.7 - the oracle does not know the flag); batches that mix flagged and
unflagged pictures; what the launch reports; the refusals of the seam on the device roads."""

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from tests import hip_harness as H
from tests import inter_stim
from tests import spec_recon
from tests import t8x8_checker as T8
from tests import synth_cases, t8x8_stim as TS

pytestmark = pytest.mark.gpu
SLOTS = 3


def wgs_and_flag(hip, batch):
    """per batch: (the k_t8x8 workgroups the launch reports, whether a picture of the batch carries the flag)"""
    return hip.last_t8x8_wgs(), any(st.pic.desc.transform_8x8 for st, _ in batch)


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    return {which: [(st, H.expect(st, T8.SpecRecon, SLOTS)) for st in getattr(TS, which)()] for which in TS.SETS}


@pytest.mark.parametrize("which", TS.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    def probe(hip, st):
        assert hip.last_t8x8_wgs() == (st.pic.mb_w * st.pic.mb_h + 7) // 8
    bad, sent = H.submit_each(lib, expected[which], SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    TS.assert_covered(which, sent)


@pytest.mark.parametrize("road", ["upload", "compact"])
def test_batches_of_three_equal_the_standard(lib, expected, road):
    cases = H.by_size(expected["directed_set"] + expected["random_set"])[(TS.MB_W, TS.MB_H)]
    bad, sent, wgs = H.run_batches(lib, cases, road=road, slots=SLOTS, probe=wgs_and_flag)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(w == 3 * ((TS.MB_W * TS.MB_H + 7) // 8) for w, _ in wgs)
    directed = {id(st.pic) for st, _ in expected["directed_set"]}
    TS.assert_covered("directed_set", [st for st in {id(st.pic): st for st in sent}.values() if id(st.pic) in directed])


def test_mixed_batches_and_what_the_launch_reports(lib, expected):
    """flagged P, flagged B, explicit-weight and unflagged pictures in one batch; a batch without a flagged picture does not
    launch k_t8x8 (and decodes as ever), one with a flagged picture does"""
    d = {st.name: (st, want) for st, want in expected["directed_set"]}
    plain = [(st, H.expect(st, spec_recon.SpecRecon, SLOTS)) for st in inter_stim.window_set()[:2] + inter_stim.b_set()[:1] + inter_stim.weighted_set()[:1]]
    assert not any(st.pic.desc.transform_8x8 for st, _ in plain)
    mixed = [d["P shapes"], plain[2], d["mixed P weighted 0"], plain[0], d["B implicit road by road"], plain[3], d["mixed B weighted 1"], plain[1], d["quadrants"]]
    bad, sent, wgs = H.run_batches(lib, mixed, slots=SLOTS, probe=wgs_and_flag)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(w > 0 for w, _ in wgs)
    kinds = {(int(st.pic.desc.slice_type), bool(st.pic.desc.explicit_wp), bool(st.pic.desc.transform_8x8)) for st in sent}
    assert kinds >= {(N.SLICE_P, False, True), (N.SLICE_B, False, True), (N.SLICE_P, True, True), (N.SLICE_P, False, False), (N.SLICE_B, False, False)}
    bad, sent, wgs = H.run_batches(lib, plain[:3], slots=SLOTS, probe=wgs_and_flag)
    assert not bad and wgs == [(0, False)]


def test_the_device_roads_refuse_what_the_seam_forbids(lib, expected):
    st, want = next(c for c in expected["directed_set"] if c[0].name.startswith("mixed P"))
    pic, rec = st.pic, st.pic.mb_records()
    fl = np.flatnonzero((rec["intra_modes"] & N.MB_T8X8) != 0)
    coded = next(int(m) for m in fl if rec["coef_mask"][m] & 0xffff)
    intra = int(np.flatnonzero(rec["mb_type"] <= N.MB_I16x16)[0])
    mask = int(rec["coef_mask"][coded])
    k = next(k for k in range(4) if mask >> (4 * k) & 1)
    assert int(pic.desc.transform_8x8) == 1
    with H.reconstructor(lib, pic.mb_w, pic.mb_h, n_streams=1, slots=SLOTS, max_pictures=2) as hip:
        H.load_frames(hip, 0, st.frames)
        H.refused_on_device_roads(lib, hip, pic, HipReconstructor.pack(pic, lib), (
            (coded, "coef_mask", mask & ~(2 << (4 * k)), 1), (intra, "intra_modes", int(rec["intra_modes"][intra]) | N.MB_T8X8, 1),
            (int(fl[0]), "qp", int(rec["qp"][fl[0]]), 0)))
        H.put(hip, lib, 0, pic, "commit")
        hip.reconstruct([0], [0])
        assert not H.differences(hip.read_frame(0, pic.desc.dst_slot), want, "the good picture behind the refused ones", pic)


# ---- a whole stream ------------------------------------------------------------------------------------------------------------
STREAM = "--mbw 8 --mbh 6 --frames 10 --refs 2 --bframes 2 --d8inf --cabac --t8x8 70 --qp 14 --qp-delta 3 --coded 35 --maxlevel 3 --seed 85"


def test_a_high_profile_cabac_b_stream_end_to_end(lib, tmp_path):
    """synth264 --t8x8 (High profile, CABAC, P and B pictures) through the parser and p264hip_submit, through the drop-in decoder
    and through the command-line decoder: every picture equals the standard's"""
    data = open(synth_cases.generate(STREAM), "rb").read()
    pics, slots, want, spec = H.parse_and_expect(lib, data, T8.SpecRecon)
    assert len(pics) == 10 and {int(p.desc.slice_type) for p in pics} == {N.SLICE_I, N.SLICE_P, N.SLICE_B}
    flagged = [int(((p.mb_records()["intra_modes"] & N.MB_T8X8) != 0).sum()) for p in pics]
    assert all(p.desc.transform_8x8 for p in pics) and sum(flagged) >= 60 and sum(f > 0 for f in flagged) >= 7, flagged
    assert spec.tells["v"] + spec.tells["h"] > 0
    H.submit_stream(lib, pics, slots, want, "p264hip_submit")
    got = H.dropin_pictures(lib, data)
    assert len(got) == 10
    H.compare_pictures(got, want, "drop-in decoder", crop=True)
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want), "the command-line decoder's pictures differ from the standard's"
