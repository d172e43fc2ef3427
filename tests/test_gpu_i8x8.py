"""Intra 8x8 macroblocks on the MI355X: the pictures of tests/i8x8_stim.py through p264hip_submit, through p264hip_upload +
p264hip_reconstruct in batches of three distinct pictures and through the compact road, all three planes byte for byte against
tests/i8x8_checker.py (H.264 8.3.2, and tests/t8x8_checker.py's residual and loop filter - the oracle does not know the flag);
which batches launch the Intra 8x8 instances of the intra kernels; mixed batches; the refusals of the seam on the device roads."""

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from tests import hip_harness as H
from tests import i8x8_checker as I8
from tests import i8x8_stim as IS
from tests import inter_stim
from tests import spec_recon
from tests import t8x8_checker as T8
from tests import synth_cases, t8x8_stim as TS

pytestmark = pytest.mark.gpu
SLOTS = 3


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    return {which: [(st, H.expect(st, I8.SpecRecon, SLOTS)) for st in getattr(IS, which)()] for which in IS.SETS}


def has_i8(st):
    return bool(int(st.pic.desc.transform_8x8) & N.T8X8_INTRA)


def launch_and_flag(hip, batch):
    """per batch: (what the launch reported, whether a picture of the batch carries N.T8X8_INTRA)"""
    return hip.last_intra_i8(), int(any(has_i8(st) for st, _ in batch))


@pytest.mark.parametrize("which", IS.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    def probe(hip, st):
        assert hip.last_intra_i8() == 1
    bad, sent = H.submit_each(lib, expected[which], SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    IS.assert_covered(which, sent)


@pytest.fixture(scope="module")
def small_dense():
    """three more dense I pictures, of the inter set's size: batches of three distinct pictures with an I picture among them"""
    rng = np.random.default_rng(8324)
    out = []
    for i in range(3):
        plan = IS.Plan(rng)
        w, h = IS.MB_W, IS.MB_H
        from tests import residual_checker as RC, seam_fuzz
        pic = seam_fuzz.make_picture(rng, w, h, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[i % 2],
                                     force={m: "i4" for m in range(w * h) if m % 5})
        RC.make_conformant(pic)
        drawn, redrawn = IS.convert(pic, rng, {m for m in range(w * h) if m % 5}, plan)
        st = IS.Stim("dense I %dx%d %d" % (w, h, i), pic, {}, drawn, redrawn)
        out.append((st, H.expect(st, I8.SpecRecon, SLOTS)))
    return out


@pytest.mark.parametrize("road", ["upload", "compact"])
def test_batches_of_three_equal_the_standard(lib, expected, small_dense, road):
    for cases in (expected["inter_set"], small_dense + expected["inter_set"][:3]):
        bad, sent, i8 = H.run_batches(lib, cases, road=road, slots=SLOTS, probe=launch_and_flag)
        assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
        assert all(got == 1 and want == 1 for got, want in i8), i8
    # the 9 x 9 picture in three streams (the band hand-over with neighbours in flight): three copies of its arrays are distinct pictures
    st, want = expected["dense_set"][0]
    rng = np.random.default_rng(8325)
    more = [IS.dense_picture(rng, IS.Plan(rng), name="dense I 9x9 b%d" % i, deblock=bool(i)) for i in range(2)]
    bad, sent, i8 = H.run_batches(lib, [(st, want)] + [(s, H.expect(s, I8.SpecRecon, SLOTS)) for s in more], road=road, slots=SLOTS, probe=launch_and_flag)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert i8 == [(1, 1)]


def plain_picture(rng, name, **kw):
    """a drawn picture of the inter set's size without any 8x8 flag, and its pictures by tests/spec_recon.py"""
    from tests import residual_checker as RC, seam_fuzz
    kw.setdefault("n_ref", 2)
    kw.setdefault("n_ref_l1", 2)
    pic = seam_fuzz.make_picture(rng, IS.MB_W, IS.MB_H, slots=SLOTS, dst_slot=0, level_style="small", qp_mode="random", mv_range=40, **kw)
    RC.make_conformant(pic)
    st = IS.Stim(name, pic, inter_stim.frames_for(rng, IS.MB_W, IS.MB_H) if kw.get("p_picture", True) else {}, 0, 0)
    return st, H.expect(st, spec_recon.SpecRecon, SLOTS)


def test_mixed_batches_and_what_the_launch_reports(lib, expected, small_dense):
    """flagged I, flagged P, a T8X8-only P and a plain B in one batch; a batch without a picture that carries N.T8X8_INTRA reports 0
    and decodes as ever"""
    rng = np.random.default_rng(8326)
    d = {st.name: (st, want) for st, want in expected["inter_set"]}
    t8 = TS.drawn_picture(rng, "P with T8X8 alone", IS.MB_W, IS.MB_H, share=0.7, intra_share=0.1, slices=1, slice_idcs=[0])
    t8_only = (t8, H.expect(t8, T8.SpecRecon, SLOTS))
    plain = [plain_picture(rng, "plain B", b_picture=True), plain_picture(rng, "plain P"), plain_picture(rng, "plain P 2", slices=2),
             plain_picture(rng, "plain I", p_picture=False)]
    assert not any(st.pic.desc.transform_8x8 for st, _ in plain) and int(t8.pic.desc.transform_8x8) == 1
    mixed = [small_dense[0], d["P cluster"], t8_only, plain[0]]
    assert [(int(st.pic.desc.slice_type), int(st.pic.desc.transform_8x8)) for st, _ in mixed] == [(N.SLICE_I, 2), (N.SLICE_P, 3), (N.SLICE_P, 1), (N.SLICE_B, 0)]
    bad, sent, i8 = H.run_batches(lib, mixed, n=4, slots=SLOTS, probe=launch_and_flag)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert i8 == [(1, 1)]
    # without a flagged picture: T8X8-only and plain pictures, plain P / B alone, a plain I picture beside them (the dense launch)
    for cases in ([t8_only, plain[0], plain[1]], plain[:3], [plain[3], plain[1], plain[2]]):
        bad, sent, i8 = H.run_batches(lib, cases, slots=SLOTS, probe=launch_and_flag)
        assert not bad and i8 == [(0, 0)], (bad[:3], i8)


def bad_records(pic):
    """(macroblock, field, value, the descriptor's transform_8x8) of the four records the seam forbids, and of the flag in pictures
    whose descriptor says 0 or 1"""
    rec = pic.mb_records()
    fl = np.flatnonzero((rec["intra_modes"] & N.MB_I8X8) != 0)
    coded = next(int(m) for m in fl if rec["coef_mask"][m] & 0xffff)
    other = int(np.flatnonzero(rec["mb_type"] != N.MB_I4x4)[0])
    mask = int(rec["coef_mask"][coded])
    k = next(k for k in range(4) if mask >> (4 * k) & 1)
    keep = int(pic.desc.transform_8x8)
    return [(other, "intra_modes", int(rec["intra_modes"][other]) | N.MB_I8X8, keep),          # not I4x4
            (coded, "coef_mask", mask & ~(2 << (4 * k)), keep),                                # a nibble of 0xD
            (coded, "intra_modes", int(rec["intra_modes"][coded]) | N.MB_T8X8, keep | 1),      # together with MB_T8X8
            (coded, "qp", int(rec["qp"][coded]), keep & ~N.T8X8_INTRA),                        # the descriptor lacks the bit
            (coded, "qp", int(rec["qp"][coded]), 0), (coded, "qp", int(rec["qp"][coded]), 1)]


def test_the_device_roads_refuse_what_the_seam_forbids(lib, expected):
    st, want = next(c for c in expected["inter_set"] if c[0].name == "P cluster")
    pic = st.pic
    with H.reconstructor(lib, pic.mb_w, pic.mb_h, n_streams=1, slots=SLOTS, max_pictures=2) as hip:
        H.load_frames(hip, 0, st.frames)
        H.refused_on_device_roads(lib, hip, pic, HipReconstructor.pack(pic, lib), bad_records(pic))
        H.put(hip, lib, 0, pic, "commit")
        hip.reconstruct([0], [0])
        assert hip.last_intra_i8() == 1
        assert not H.differences(hip.read_frame(0, pic.desc.dst_slot), want, "the good picture behind the refused ones", pic)


# ---- a whole stream ------------------------------------------------------------------------------------------------------------
STREAM = "--mbw 8 --mbh 6 --frames 10 --refs 2 --bframes 2 --d8inf --cabac --t8x8 60 --i8x8 60 --intra-pct 25 --qp 14 --qp-delta 3 --coded 35 --maxlevel 3 --seed 86"


def test_a_high_profile_cabac_stream_with_intra_8x8_end_to_end(lib, tmp_path):
    """synth264 --cabac --t8x8 60 --i8x8 60 (I, P and B pictures) through the parser and p264hip_submit, through the drop-in decoder
    and through the command-line decoder: every picture equals the standard's"""
    data = open(synth_cases.generate(STREAM), "rb").read()
    pics, slots, want, spec = H.parse_and_expect(lib, data, I8.SpecRecon, intra8x8=True)
    assert len(pics) == 10 and {int(p.desc.slice_type) for p in pics} == {N.SLICE_I, N.SLICE_P, N.SLICE_B}
    flagged = [int(((p.mb_records()["intra_modes"] & N.MB_I8X8) != 0).sum()) for p in pics]
    assert spec.met >= 7 and sum(f > 0 for f in flagged) == spec.met and sum(flagged) >= 30, flagged
    assert any((p.mb_records()["intra_modes"] & N.MB_T8X8).any() for p in pics)
    assert len(spec.census8.blocks) >= 30 and spec.tells["v"] + spec.tells["h"] > 0
    def probe(hip, i, p):
        assert hip.last_intra_i8() == int(flagged[i] > 0)
    H.submit_stream(lib, pics, slots, want, "p264hip_submit", probe)
    got = H.dropin_pictures(lib, data)
    assert len(got) == 10
    H.compare_pictures(got, want, "drop-in decoder", crop=True)
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want), "the command-line decoder's pictures differ from the standard's"
