"""Per-macroblock filter offsets (`flags`, include/p264hip.h) on the MI355X: the families of tests/slice_filter_fuzz.py - pictures
of seam_fuzz.make_picture (P, B, I, sliced, lists that hold a frame twice, explicit weights, I_PCM), deltas per slice run or per
macroblock over the whole int8 range or over -12 .. 12, next to pictures without deltas in the same launch - against the oracle's
unfiltered reconstruction followed by tests/slice_filter_checker.py.  Bytes of all three planes, every picture, no tolerance.

Every family goes through the compact upload and one p264hip_reconstruct call (one stream per picture), and picture by picture
through p264hip_submit; the launch info says which edge-info instance ran (the role fused into k_intra_sparse, k_deblock_bs<false>,
k_deblock_bs<true>).  Three families - one per instance - repeat at the launch shapes of tests/test_gpu_batch_shapes.py.  What the
comparisons cover is asserted on the CPU (tests/test_slice_filter_cpu.py::test_coverage_of_the_drawn_families).

All of it fails on kernels that ignore `flags`: the pictures with deltas come out filtered with the picture's offsets."""
import pytest

from tests import slice_filter_fuzz as sff
from tests.stream_args import LAUNCH_SHAPES as SHAPES
from tests.hip_harness import ROADS, compare, load_frames, put, reconstructor

pytestmark = pytest.mark.gpu


def check_instance(name, li):
    instance = sff.FAMILIES[name][2]
    assert (li["edge_info_fused"] > 0) == (instance == "fused"), (name, li)


def run_family(lib, oracle, name, road):
    mb_w, mb_h, instance, _ = sff.FAMILIES[name]
    cases, counts = sff.family(oracle, name)
    n = len(cases)
    with reconstructor(lib, mb_w, mb_h, n_streams=n, slots=sff.SLOTS, max_pictures=n) as hip:
        for s, c in enumerate(cases):
            load_frames(hip, s, c.refs)
        if road == "compact":
            for s, c in enumerate(cases):
                put(hip, lib, s, c.pic, "compact")
            hip.reconstruct(list(range(n)), list(range(n)))
            li = hip.last_launch()
            assert li["pictures"] == n
            check_instance(name, li)
            for s, c in enumerate(cases):
                compare(hip.read_frame(s, sff.DST), c.want, "%s stream %d of %d, compact upload, deltas %s" % (name, s, n, c.mode), c.pic)
        else:
            for s, c in enumerate(cases):
                hip.submit(s, c.pic)
                compare(hip.read_frame(s, sff.DST), c.want, "%s stream %d, p264hip_submit, deltas %s" % (name, s, c.mode), c.pic)
        hip.sync()


@pytest.mark.parametrize("road", ["compact", "submit"])
@pytest.mark.parametrize("name", list(sff.FAMILIES))
def test_slice_filter_fuzz(lib, oracle, name, road):
    run_family(lib, oracle, name, road)


@pytest.mark.parametrize("rb,per_wg,intra_waves", SHAPES)
@pytest.mark.parametrize("name", ["p_plain", "p_with_i", "b_mix"])
def test_slice_filter_fuzz_at_every_launch_shape(lib, oracle, name, rb, per_wg, intra_waves, monkeypatch):
    monkeypatch.setenv("P264AMD_DEBLOCK_RB_LOG2", rb)
    monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)
    monkeypatch.setenv("P264AMD_INTRA_WAVES", intra_waves)
    run_family(lib, oracle, name, "compact")


@pytest.mark.parametrize("name", ["b_mix", "pcm_p"])
def test_every_road_into_a_slot_carries_the_deltas(lib, oracle, name):
    """plain upload, the packed block, the compact block, reserve / commit (the device's record check in front of the launch) and
    p264hip_clone_picture - the picture of stream s goes in by road s % 5, all in one launch"""
    mb_w, mb_h, instance, _ = sff.FAMILIES[name]
    cases, _ = sff.family(oracle, name)
    n = len(cases)
    with reconstructor(lib, mb_w, mb_h, n_streams=n, slots=sff.SLOTS, max_pictures=2 * n) as hip:
        roads = []
        for s, c in enumerate(cases):
            load_frames(hip, s, c.refs)
            road = (ROADS + ("clone",))[s % 5]
            roads.append(road)
            if road == "clone":
                hip.upload(n + s, [c.pic])
                hip.clone_picture(s, n + s)
            else:
                put(hip, lib, s, c.pic, road)
        assert len(set(roads)) == min(n, 5)
        hip.reconstruct(list(range(n)), list(range(n)))
        check_instance(name, hip.last_launch())
        for s, c in enumerate(cases):
            compare(hip.read_frame(s, sff.DST), c.want, "%s stream %d by %s, deltas %s" % (name, s, roads[s], c.mode), c.pic)
        hip.sync()
