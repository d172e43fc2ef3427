"""A Cr QP offset of its own (p264hip_picture_t.cr_qp_offset_delta) on the MI355X: the directed pictures of tests/cr_offset_stim.py -
I, P with sparse intra and B at 1 x 1, 2 x 5, 9 x 1, 11 x 9 and 70 x 3, every pair of chroma_qp_offset -12 / 0 / 12 and delta -24 /
-13 / -1 / +1 / +7 / +24, with scaling lists, P264_MB_T8X8, P264_MB_I8X8, explicit weights, I_PCM macroblocks and with deblock = 0 -
through p264hip_submit and through every road into an input slot, all three planes byte for byte against the two-chain composite of
tests/cr_offset_checker.py (Y and U of the picture decoded with Cb's offset, V of the picture decoded with Cr's); what the launch reports."""
import pytest

from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import hip_harness as H
from tests import scaling_checker as SC

pytestmark = pytest.mark.gpu


def expect(st):
    two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, CS.SLOTS)
    for slot, f in st.frames.items():
        two.store.write(slot, f)
    want = two.reconstruct(st.pic)
    assert two.v_differs == 1, "%s: Cr's offset changes nothing" % st.name
    return want


@pytest.fixture(scope="module")
def expected():
    return [(st, expect(st)) for st in CS.directed_set()]


def test_submit_equals_the_composite(lib, expected):
    def probe(hip, st):
        assert (hip.last_cr_pictures(), hip.last_scaled_pictures(), hip.last_t8x8_wgs()) == (1, 1, 0), st.name
        assert hip.last_launch()["edge_info_fused"] == 0
    bad, sent = H.submit_each(lib, expected, CS.SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert len(sent) == len(expected) >= 20


ROAD_PICTURES = ("I 2x5", "P 11x9", "B 11x9", "P 70x3", "lists P", "T8X8 B", "I8X8 P", "weighted B", "I_PCM P", "unfiltered P")


@pytest.mark.parametrize("which", ROAD_PICTURES)
def test_every_road_into_a_slot_carries_the_delta(lib, expected, which):
    """upload, packed, compact, reserve / commit, and a clone of the slot: the same bytes every time"""
    (st, want), = [(st, want) for st, want in expected if st.name.startswith(which + " ")]
    pic = st.pic
    with H.reconstructor(lib, pic.mb_w, pic.mb_h, n_streams=2, slots=CS.SLOTS, max_pictures=2) as hip:
        for k in range(2):
            H.load_frames(hip, k, st.frames)
        H.through_roads(hip, lib, pic, want, st.name, H.ROADS)
        assert (hip.last_cr_pictures(), hip.last_scaled_pictures()) == (1, 1)
        for road in ("upload", "compact"):
            H.put(hip, lib, 0, pic, road)
            hip.clone_picture(1, 0)
            hip.reconstruct([1], [1])
            assert hip.last_cr_pictures() == 1
            H.compare(hip.read_frame(1, pic.desc.dst_slot), want, "%s (a clone behind %s)" % (st.name, road), pic)
        hip.sync()
