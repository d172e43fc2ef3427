"""Reference lists of up to 16 entries in frame stores of 17 slots, on the GPU.

tests/long_lists_stim.py draws the pictures (8 x 6 macroblocks; tests/test_long_lists_cpu.py shows what the set reaches and that every
picture tells a decoder that drops bit 3 of an index, mixes the lists' slots, transposes the implicit weights, takes the explicit
weights of `index & 7` or compares indices where H.264 8.7.2.1 compares pictures).  Here every picture goes through p264hip_submit,
through batches of three distinct pictures on the upload road and one batch each on the packed, compact and commit roads, and through
one mixed batch of P, B, weighted and scaled pictures; all three planes are compared byte for byte with tests/spec_recon.py (the three
kinds that are there for a kernel instance: with the checker of what selects it), and the launch must report what the batch's kinds
imply (tests/batch_kinds.py: plan_rules).  Then the store itself: 17 slots accepted, 18 refused, a store past the per-stream bound
refused before anything is allocated, every slot of two streams written and read back, slot 16 exported and resized, a cloned
16-entry picture."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import batch_kinds as BK
from tests import hip_harness as H
from tests import long_lists_stim as LS
from tests import seam_fuzz

pytestmark = pytest.mark.gpu

SORT = {"plain": "k_mc_sort", "wp": "k_mc_sort_wp", "b": "k_mc_sort_b", "b_wp": "k_mc_sort_b_wp", "scaled_p": "k_mc_sort_scaled_p", "scaled": "k_mc_sort_scaled"}
EDGE = {"fused": "k_intra_sparse (edge info)", "bs_true": "k_deblock_bs (by picture table)", "bs_false": "k_deblock_bs (plain P)"}
EVERY_INSTANCE = set(SORT.values()) | {"k_mc", "k_mc_wp", "k_mc_second", "k_deblock_bs_cr"} | set(EDGE.values())
ROAD_BATCHES = {"packed": ("P 16", "B 16+16", "P wp 16"), "compact": ("B wp 16+16", "B implicit 16+16", "P dup 16"),
                "commit": ("B lists 16+16", "P t8 16", "B 1+16")}
MIXED = ("P 16", "B implicit 16+16", "P wp 16", "B wp 16+16", "P lists 16", "B lists 16+16", "P cr 16", "P t8 16", "P dup 16", "B implicit 9+7")


@pytest.fixture(scope="module")
def cases():
    """[(stimulus, [y, u, v] by the standard)], computed once"""
    return [(st, LS.expected(st)) for st in LS.pictures()]


def instances(hip, pics, what):
    """the launch's report against what the pictures' kinds imply (as tests/test_gpu_batch_kinds.py reads it); the names of the
    instances the plan's rules give this batch"""
    from tests.test_gpu_batch_kinds import check_report
    e = BK.plan_rules(BK.union(BK.flags_of(p) for p in pics), len(pics), None, LS.W * LS.H)
    check_report(hip, e, what)
    ran = {SORT[e["sort"]], "k_mc_wp" if e["mc"] == "wp" else "k_mc", EDGE[e["edge"]]}
    if e["second"]:
        ran.add("k_mc_second")
    if e["deblock_cr"]:
        ran.add("k_deblock_bs_cr")
    return ran


def test_submit_equals_the_standard(lib, cases):
    ran = {}

    def probe(hip, st):
        ran[st.name] = instances(hip, [st.pic], st.name)
    bad, sent = H.submit_each(lib, cases, LS.SLOTS, probe)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    LS.assert_covered(sent)
    for name, inst in sorted(ran.items()):
        print("%-24s %s" % (name, sorted(inst)))
    assert set().union(*ran.values()) == EVERY_INSTANCE, sorted(EVERY_INSTANCE - set().union(*ran.values()))
    # the pictures that are there for an instance ran it, with 16-entry lists
    assert "k_mc_sort_scaled_p" in ran["P lists 16"] and "k_mc_sort_scaled" in ran["B lists 16+16"] and "k_deblock_bs_cr" in ran["P cr 16"]
    assert EDGE["fused"] in ran["P 16"] and EDGE["bs_true"] in ran["P dup 16"] and "k_mc_sort_b_wp" in ran["B wp 16+16"]


@pytest.mark.parametrize("road", H.ROADS)
def test_batches_of_three_equal_the_standard(lib, cases, road):
    if road == "upload":
        mine = cases
    else:
        mine = [c for name in ROAD_BATCHES[road] for c in cases if c[0].name == name]
        assert len(mine) == 3
    bad, sent, probed = H.run_batches(lib, mine, 3, road, LS.SLOTS, lambda hip, batch: instances(hip, [st.pic for st, _ in batch], road))
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert len(sent) >= len(mine) and {st.name for st in sent} == {st.name for st, _ in mine}
    if road == "upload":
        LS.assert_covered(sent)
        # (three pictures share a launch: the scaled P sort and the plain-P strengths pass need a batch of their kind alone)
        assert set().union(*probed) >= EVERY_INSTANCE - {EDGE["bs_false"], "k_mc_sort_scaled_p"}


def test_one_mixed_batch(lib, cases):
    """P, B, weighted and scaled pictures in one call: the batch picks the scaled sort, k_mc_wp and the second pass for all of them"""
    mine = [c for name in MIXED for c in cases if c[0].name == name]
    n = len(mine)
    assert n == len(MIXED)
    with H.reconstructor(lib, LS.W, LS.H, n_streams=n, slots=LS.SLOTS, max_pictures=n) as hip:
        for k, (st, _) in enumerate(mine):
            H.load_frames(hip, k, st.frames)
        hip.upload(0, [st.pic for st, _ in mine])
        hip.reconstruct(list(range(n)), list(range(n)))
        ran = instances(hip, [st.pic for st, _ in mine], "the mixed batch")
        assert ran == {"k_mc_sort_scaled", "k_mc_wp", "k_mc_second", "k_deblock_bs_cr", EDGE["bs_true"]}
        assert hip.last_scaled_pictures() == 3 and hip.last_cr_pictures() == 1 and hip.last_t8x8_wgs() == 0      # (scaled batches run k_scaled_inter instead)
        bad = []
        for k, (st, want) in enumerate(mine):
            bad += H.differences(hip.read_frame(k, st.pic.desc.dst_slot), want, "%s (stream %d of the mixed batch)" % (st.name, k), st.pic)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), n, bad[:3])


# ---- the store's seventeen slots ---------------------------------------------------------------------------------------------------
def test_create_takes_17_slots_and_refuses_18(lib):
    assert N.MAX_REFS == 16 and LS.SLOTS == N.MAX_REFS + 1
    with H.reconstructor(lib, LS.W, LS.H, n_streams=1, slots=17, max_pictures=1) as hip:
        assert hip.slots == 17
    ctx = C.c_void_p()
    assert lib.p264hip_create(C.byref(ctx), 0, LS.W, LS.H, 1, 18, 1) == -1 and not ctx.value          # P264HIP_EINVAL
    assert b"bad argument" in lib.p264hip_last_error()


def test_a_store_past_the_bound_is_refused_before_anything_is_allocated(lib):
    """the largest geometry with 17 slots: 17 frames of 402 MB are past what one stream's 32-bit offsets address"""
    lib.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert lib.hipDeviceSynchronize() == 0 and lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    with H.reconstructor(lib, LS.W, LS.H, n_streams=1, slots=17, max_pictures=1):      # (the runtime is up: what follows measures the call alone)
        before = free_bytes()
        ctx = C.c_void_p()
        assert lib.p264hip_create(C.byref(ctx), 0, 2047, 512, 1, 17, 1) == -1 and not ctx.value
        assert b"frame store of one stream exceeds" in lib.p264hip_last_error()
        assert free_bytes() == before
    # (the same geometry with the slots that fit is a matter of memory, not of this bound: tests/test_gpu_limit_geometry.py)
    frame = 2047 * 512 * 384
    assert 17 * frame > 0xffffff00 >= 10 * frame


def test_every_slot_of_two_streams_keeps_its_frame(lib):
    rng = np.random.default_rng(1716)
    with H.reconstructor(lib, LS.W, LS.H, n_streams=2, slots=17, max_pictures=1) as hip:
        frames = {(s, k): seam_fuzz.random_frame(rng, LS.W, LS.H) for s in (0, 1) for k in range(17)}
        for (s, k), f in frames.items():
            hip.write_frame(s, k, *f)
        for (s, k), f in sorted(frames.items(), reverse=True):
            H.compare(hip.read_frame(s, k), f, "stream %d slot %d" % (s, k))
        # a slot rewritten leaves its neighbours alone
        again = seam_fuzz.random_frame(rng, LS.W, LS.H)
        hip.write_frame(0, 16, *again)
        frames[(0, 16)] = again
        for key in ((0, 15), (0, 16), (1, 0), (1, 16)):
            H.compare(hip.read_frame(*key), frames[key], "stream %d slot %d after a write to (0, 16)" % key)


def test_slot_16_of_stream_1_out_and_resized(lib):
    from tests.test_gpu_export import run as run_export
    from tests.test_gpu_resize import run as run_resized
    rng = np.random.default_rng(1717)
    w, h = LS.W * 16, LS.H * 16
    with H.reconstructor(lib, LS.W, LS.H, n_streams=2, slots=17, max_pictures=1) as hip:
        planes = {(s, k): seam_fuzz.random_frame(rng, LS.W, LS.H, "smooth") for s, k in ((0, 0), (0, 16), (1, 0), (1, 15), (1, 16))}
        for (s, k), f in planes.items():
            hip.write_frame(s, k, *f)
        for streams, slots in (([1], [16]), ([0, 1, 1], [16, 16, 15])):
            got, want = run_export(hip, planes, streams, slots, "nv12", (0, 0, w, h))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "export of %s / %s: %d bytes differ, the first at %d" % (streams, slots, bad.size, bad[0])
            got, want = run_resized(hip, planes, streams, slots, "rgbp", (2, 2, w - 4, h - 4), (64, 48))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "resize of %s / %s: %d bytes differ, the first at %d" % (streams, slots, bad.size, bad[0])


@pytest.mark.parametrize("name", ["B implicit 16+16", "P wp 16"])
def test_a_cloned_picture_decodes_to_the_same_bytes(lib, cases, name):
    st, want = next(c for c in cases if c[0].name == name)
    dst = int(st.pic.desc.dst_slot)
    with H.reconstructor(lib, LS.W, LS.H, n_streams=2, slots=17, max_pictures=2) as hip:
        for s in (0, 1):
            H.load_frames(hip, s, st.frames)
        for road in ("upload", "compact"):
            H.put(hip, lib, 0, st.pic, road)
            hip.clone_picture(1, 0)
            hip.reconstruct([0, 1], [0, 1])
            for s in (0, 1):
                H.compare(hip.read_frame(s, dst), want, "%s (%s behind %s)" % (name, "the clone" if s else "the original", road), st.pic)
                hip.write_frame(s, dst, *st.frames[dst])
        hip.sync()
