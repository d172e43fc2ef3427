"""Pictures with a Cr QP offset of their own among flat, scaled and delta-0 pictures, in batches of 1, 2, 3 and 5, under the loop
filter's shape knobs (bands of 4 and 8 rows, several pictures per workgroup, the odd-single shape, fewer wavefronts than units): a
batch that holds such a picture runs the Cr instances for ALL its pictures - the flat ones with delta 0 must come out as they do alone,
which is what their expectation (tests/scaling_checker.py) says; a batch without one reports cr_pictures == 0."""
import pytest

from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import hip_harness as H
from tests import scaling_checker as SC
from tests.test_gpu_cr_offset import expect

pytestmark = pytest.mark.gpu

RB, PER_WG, ODD, WAVES = "P264AMD_DEBLOCK_RB_LOG2", "P264AMD_DEBLOCK_PICS_PER_WG", "P264AMD_DEBLOCK_ODD_SINGLE", "P264AMD_DEBLOCK_WAVES"
KNOBS = {"built-in": {}, "bands of 4 rows, pairs": {RB: "2", PER_WG: "2"}, "bands of 8 rows": {RB: "3", PER_WG: "1"},
         "five per workgroup": {RB: "2", PER_WG: "5"}, "three per workgroup in bands of 8": {RB: "3", PER_WG: "3"},
         "odd single": {RB: "2", PER_WG: "3", ODD: "1"}, "one wavefront": {RB: "2", PER_WG: "4", WAVES: "1"},
         "two wavefronts": {RB: "3", PER_WG: "5", WAVES: "2"}}


@pytest.fixture(scope="module")
def cases():
    """delta and delta-0 pictures taking turns: every batch of two or more holds both"""
    with_delta, without = CS.batch_set(), CS.flat_set()
    mixed = [st for pair in zip(with_delta, without) for st in pair]
    assert [CR.delta_of(st.pic) != 0 for st in mixed] == [True, False] * 4
    return [(st, expect(st) if CR.delta_of(st.pic) else H.expect(st, SC.SpecRecon, CS.SLOTS)) for st in mixed]


def counts(hip, batch):
    want_cr = sum(CR.delta_of(st.pic) != 0 for st, _ in batch)
    want_sc = sum(CR.delta_of(st.pic) != 0 or bool(int(st.pic.desc.scaling_lists)) for st, _ in batch)
    return (hip.last_cr_pictures(), hip.last_scaled_pictures()), (want_cr, want_sc), hip.last_launch()


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("knobs", list(KNOBS))
def test_mixed_batches_at_every_deblock_shape(lib, cases, knobs, n, monkeypatch):
    for k, v in KNOBS[knobs].items():
        monkeypatch.setenv(k, v)
    bad, sent, seen = H.run_batches(lib, cases, n=n, slots=CS.SLOTS, probe=counts)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(got == want for got, want, _ in seen), [(got, want) for got, want, _ in seen]
    assert any(got[0] for got, _, _ in seen) and (n == 1 or all(0 < got[0] < n for got, _, _ in seen))
    for _, _, li in seen:
        if RB in KNOBS[knobs]:
            assert (li["deblock_rb_log2"], li["deblock_pics_per_wg"]) == (int(KNOBS[knobs][RB]), int(KNOBS[knobs][PER_WG])), li
        if ODD in KNOBS[knobs]:
            assert li["deblock_odd_single"] == 1, li


@pytest.mark.parametrize("road", ["compact", "commit"])
def test_mixed_batches_through_the_other_roads(lib, cases, road):
    bad, sent, seen = H.run_batches(lib, cases, n=3, road=road, slots=CS.SLOTS, probe=counts)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(got == want for got, want, _ in seen)


def test_a_batch_without_a_delta_is_what_it_was(lib, cases):
    """no picture with a delta: cr_pictures 0, scaled_pictures counts the lists alone, and the shapes are those of the same batch
    with a delta picture in it (the Cr instances take the same roads and shapes)"""
    flat = [(st, want) for st, want in cases if not CR.delta_of(st.pic)]
    bad, sent, seen = H.run_batches(lib, flat, n=len(flat), slots=CS.SLOTS, probe=counts)
    assert not bad, bad[:3]
    (got, want, li), = seen
    assert got == want == (0, 1), (got, want)
    mixed = flat[:-1] + [c for c in cases if CR.delta_of(c[0].pic) and int(c[0].pic.desc.slice_type) == int(flat[-1][0].pic.desc.slice_type)][:1]
    bad, sent, seen = H.run_batches(lib, mixed, n=len(mixed), slots=CS.SLOTS, probe=counts)
    assert not bad, bad[:3]
    assert seen[0][0] == (1, 2) and seen[0][2] == li, (seen[0], li)
