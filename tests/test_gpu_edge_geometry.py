"""The High-profile kernel instances at the edge geometries, on the MI355X: the pictures of tests/edge_geometry_stim.py - 1 x 1, 1 x 7,
2 x 5, 9 x 1, 70 x 3 and 66 x 5 macroblocks; flat and scaled, P / B / I, Intra 8x8 macroblocks and T8X8 inter records - one by one through
p264hip_submit and in batches of distinct pictures through the upload and compact roads: batches of three as they come (flat beside
scaled), the flat pictures alone (k_t8x8, k_intra_i8 / k_intra_sparse_i8) and the scaled ones alone (k_scaled_inter, k_intra_scaled /
k_intra_sparse_scaled).  All three planes byte for byte against tests/scaling_checker.py's SpecRecon (H.264 8.3.2, 8.5.9 - 8.5.13), and
what each launch reports.  The expected pictures are computed once per module.  The four small geometries also as whole streams
(synth264: CABAC, I + P + B, the 8x8 transform in inter and intra macroblocks, flat and with scaling matrices) through the parser and
p264hip_submit; at 70 x 3 such a stream always holds a macroblock outside the range of 8.5.13, which is why the pictures above are drawn
at the seam."""
import pytest

from p264decoder_amd import _native as N
from tests import edge_geometry_stim as E
from tests import hip_harness as H
from tests import scaling_checker as SC
from tests import synth_cases

pytestmark = pytest.mark.gpu
SLOTS = 3
IDS = lambda g: "%dx%d" % g


@pytest.fixture(scope="module")
def expected():
    """{geometry: [(stim, [y, u, v] by the standard)]}, flat pictures first"""
    return {g: [(st, H.expect(st, SC.SpecRecon, SLOTS)) for st in E.picture_set(*g)] for g in E.GEOMETRIES}


def t8x8_wgs_of(batch, geometry):
    """what last_t8x8_wgs must report: ceil(n_mb / 8) workgroups per picture of a flat batch that holds a picture with T8X8 records, 0 next to a
    scaled picture (k_scaled_inter owns the batch's 8x8 blocks then)"""
    stims = [st for st, _ in batch]
    if any(E.is_scaled(st) for st in stims) or not any(E.runs_k_t8x8(st) for st in stims):
        return 0
    return -(-geometry[0] * geometry[1] // 8) * len(stims)


def launch_facts(geometry):
    def probe(hip, batch):
        got = (hip.last_intra_i8(), hip.last_scaled_pictures(), hip.last_t8x8_wgs())
        want = (1, sum(E.is_scaled(st) for st, _ in batch), t8x8_wgs_of(batch, geometry))
        return got, want
    return probe


@pytest.mark.parametrize("geometry", E.GEOMETRIES, ids=IDS)
def test_submit_equals_the_standard(lib, expected, geometry):
    facts = launch_facts(geometry)

    def probe(hip, st):
        got, want = facts(hip, [(st, None)])
        assert got == want, "%s: (intra_i8, scaled pictures, k_t8x8 workgroups) %s, expected %s" % (st.name, got, want)
    bad, sent = H.submit_each(lib, expected[geometry], SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    E.assert_covered(geometry, sent)


@pytest.mark.parametrize("road", ["upload", "compact"])
@pytest.mark.parametrize("geometry", E.GEOMETRIES, ids=IDS)
def test_batches_equal_the_standard(lib, expected, geometry, road):
    cases = expected[geometry]
    flat, scaled = [c for c in cases if not E.is_scaled(c[0])], [c for c in cases if E.is_scaled(c[0])]
    assert len(flat) >= 2 and len(scaled) >= 3 and any(E.runs_k_t8x8(st) for st, _ in flat)
    mixed = [c for pair in zip(scaled, flat) for c in pair] + scaled[len(flat):] + flat[len(scaled):]      # scaled, flat, scaled, flat ..
    sent_all = []
    # batches of three distinct pictures, each with flat and scaled ones; the flat pictures in one batch; the scaled ones in one batch
    for what, batch, n in (("mixed", mixed, 3), ("flat", flat, len(flat)), ("scaled", scaled, len(scaled))):
        bad, sent, facts = H.run_batches(lib, batch, n=n, road=road, slots=SLOTS, probe=launch_facts(geometry))
        assert not bad, "%s batches: %d of %d pictures differ: %s" % (what, len(bad), len(sent), bad[:3])
        assert all(got == want for got, want in facts), "%s batches: (intra_i8, scaled pictures, k_t8x8 workgroups) and what was expected: %s" % (what, facts)
        counts = [want[1] for _, want in facts]
        assert all(0 < c < 3 for c in counts) if what == "mixed" else counts == [0 if what == "flat" else n], (what, counts)
        if what == "flat":
            assert facts[0][1][2] == -(-geometry[0] * geometry[1] // 8) * n > 0
        sent_all += sent
    E.assert_covered(geometry, list({id(st.pic): st for st in sent_all}.values()))


STREAM = "--mbw %d --mbh %d --frames 8 --refs 2 --bframes 2 --d8inf --cabac --t8x8 70 --i8x8 50 --qp 14 --qp-delta 3 --coded 35 --maxlevel %d --seed %d %s"
CQM = {"flat": (3, ""), "jvt in the sps": (3, "--cqm jvt --cqm-where sps"), "random lists in both sets": (2, "--cqm rand:7 --cqm-where both")}


@pytest.mark.parametrize("cqm", list(CQM))
@pytest.mark.parametrize("geometry", [g for g in E.GEOMETRIES if g[0] <= E.WINDOW], ids=IDS)
def test_a_high_profile_stream_of_a_small_geometry(lib, geometry, cqm):
    maxlevel, args = CQM[cqm]
    data = open(synth_cases.generate(STREAM % (geometry[0], geometry[1], maxlevel, 90 + E.GEOMETRIES.index(geometry), args)), "rb").read()
    pics, slots, want, spec = H.parse_and_expect(lib, data, SC.SpecRecon, intra8x8=True, scaling=True)
    scaled = cqm != "flat"
    assert len(pics) == 8 and (pics[0].mb_w, pics[0].mb_h) == geometry and spec.scaled == (8 if scaled else 0)
    assert {int(p.desc.slice_type) for p in pics} == {N.SLICE_I, N.SLICE_P, N.SLICE_B}
    for i, p in enumerate(pics):
        n, out = SC.census(p)
        assert not out, "picture %d: %d level blocks feed a value out of range: %s" % (i, len(out), sorted(out)[:3])
    t8 = sum(int(((p.mb_records()["intra_modes"] & N.MB_T8X8) != 0).sum()) for p in pics)
    i8 = sum(int(((p.mb_records()["intra_modes"] & N.MB_I8X8) != 0).sum()) for p in pics)
    assert t8 >= 1 and i8 >= 1 and any(int(p.desc.transform_8x8) & N.T8X8_INTRA for p in pics), (t8, i8)

    def probe(hip, i, p):
        assert hip.last_scaled_pictures() == int(scaled) and hip.last_intra_i8() == int(bool(int(p.desc.transform_8x8) & N.T8X8_INTRA))
    H.submit_stream(lib, pics, slots, want, "%dx%d %s" % (geometry + (cqm,)), probe)
