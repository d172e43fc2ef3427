"""Decoding at the geometries where the kernels change path and at the limits of the context, on the MI355X: the pictures of
tests/limit_geometry.py - 1 x 160, 1 x 161, 65 x 81, 64 x 128, 64 x 129, 33 x 32, 3 x 512 and 2047 x 2 macroblocks - byte for byte
against their expectations (the oracle; tests/wp_checker.py for explicit weights; SHA-256 per plane from
tests/golden/limit_geometry.json where the checker is slow: that module says which is which), alone through p264hip_submit, in batches
that select every sort, motion-compensation, intra and edge-info instance of the Baseline / Main kinds (one reconstruct call each, the
launch report checked against tests/batch_kinds.py's rules) and through the roads into an input slot; pictures with T8X8 records and
Intra 8x8 macroblocks, flat and scaled, the same way on every geometry above 161 macroblocks; the limit vectors that land
inside a picture 32752 samples wide or 8192 tall; the tall pictures through the loop filter's band shapes and the intra kernels'
wavefront counts; frames out and resized from the far end of such a frame; what p264hip_create refuses and the extremes it accepts.

A wait inside the kernels is bounded (SPIN_LIMIT) and surfaces as an error of reconstruct: a test that fails that way is a finding to
be read from the code."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from p264decoder_amd.recon import P264Error
from tests import batch_kinds as BK
from tests import edge_geometry_stim as E
from tests import export_checker as X
from tests import hip_harness as H
from tests import limit_geometry as L
from tests import seam_fuzz
from tests.test_gpu_batch_kinds import check_report

pytestmark = pytest.mark.gpu
K = "P264AMD_"
# the batches of the Baseline / Main kinds, by what they make the plan choose (sort, mc, second pass, intra, edge-info road)
BATCHES = {("P", "I"): ("plain", "plain", 0, "dense", "bs_false"), ("P", "B implicit"): ("b", "plain", 1, "sparse", "bs_true"),
           ("P weighted", "P"): ("wp", "wp", 0, "sparse", "bs_true"), ("B weighted", "I", "P"): ("b_wp", "wp", 1, "dense", "bs_true"),
           ("B implicit", "P weighted", "B weighted", "I", "P"): ("b_wp", "wp", 1, "dense", "bs_true")}
ALONE = {"P": ("plain", "plain", 0, "sparse", "fused"), "I": ("none", "none", 0, "dense", "bs_false"), "B implicit": ("b", "plain", 1, "sparse", "bs_true"),
         "P weighted": ("wp", "wp", 0, "sparse", "bs_true"), "B weighted": ("b_wp", "wp", 1, "sparse", "bs_true")}


def same(got, want, what, pic=None):
    """[] or [a message]: planes against planes, or against the golden file's SHA-256 per plane"""
    if isinstance(want[0], str):
        bad = [i for i, (a, b) in enumerate(zip(L.plane_hashes(got), want)) if a != b]
        return ["%s: planes %s differ from the golden file's" % (what, bad)] if bad else []
    return H.differences(got, want, what, pic)


@pytest.fixture(scope="module")
def cases(oracle):
    """cases(geometry) -> {kind: (stimulus, planes or hashes)} of main_set, and of the scaled / Cr picture where the geometry has one;
    computed once per geometry"""
    memo = {}

    def of(geometry):
        if geometry not in memo:
            out = {k: (st, L.expected(oracle, st, L.main_key(geometry, k))) for k, st in L.main_set(geometry).items()}
            if geometry in L.SCALED_GEOMETRIES:
                st = L.scaled_picture(geometry)
                out["scaled P"] = (st, L.expected(oracle, st, "%s/scaled P" % L.IDS(geometry)))
            if geometry in L.CR_GEOMETRIES:
                st = L.cr_picture(geometry)
                out["Cr P"] = (st, L.expected(oracle, st, "%s/Cr P" % L.IDS(geometry)))
            memo[geometry] = out
        return memo[geometry]
    return of


def plan_of(members, geometry):
    """the plan's report and instance tuple for a batch of these stimuli (tests/batch_kinds.py: flags_of, plan_rules)"""
    e = BK.plan_rules(BK.union(BK.flags_of(st.pic) for st in members), len(members), None, geometry[0] * geometry[1])
    return e, (e["sort"], e["mc"], e["second"], e["intra"], e["edge"])


def run_batch(hip, members, geometry, what):
    """the (stimulus, expectation) pairs in ONE reconstruct call, each on its own stream; the launch report checked; the differences"""
    n = len(members)
    for k, (st, want) in enumerate(members):
        H.load_frames(hip, k, st.frames)
        hip.write_frame(k, L.DST, *[np.zeros((geometry[1] * 16 >> (i > 0), geometry[0] * 16 >> (i > 0)), np.uint8) for i in range(3)])
    hip.upload(0, [st.pic for st, _ in members])
    hip.reconstruct(list(range(n)), list(range(n)))
    e, tup = plan_of([st for st, _ in members], geometry)
    check_report(hip, e, what)
    bad = []
    for k, (st, want) in enumerate(members):
        bad += same(hip.read_frame(k, L.DST), want, "%s, %s" % (st.name, what), st.pic)
    return bad, tup


@pytest.mark.parametrize("geometry", L.GEOMETRIES, ids=L.IDS)
def test_every_kind_alone(lib, cases, geometry):
    kinds = cases(geometry)
    L.assert_covered(geometry, {k: kinds[k][0] for k in L.MAIN})
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=1, slots=L.SLOTS, max_pictures=1) as hip:
        for k, (st, want) in kinds.items():
            H.load_frames(hip, 0, st.frames)
            hip.submit(0, st.pic)
            e, tup = plan_of([st], geometry)
            check_report(hip, e, st.name)
            if k in ALONE:
                assert tup == ALONE[k], (k, tup)
            else:
                assert tup[0] == "scaled_p" and tup[3] == "sparse_scaled" and e["cr_pictures"] == int(k == "Cr P"), (k, tup, e)
            bad += same(hip.read_frame(0, L.DST), want, st.name, st.pic)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(kinds), bad[:3])


@pytest.mark.parametrize("geometry", L.GEOMETRIES, ids=L.IDS)
def test_batches_select_every_instance(lib, cases, geometry):
    kinds = cases(geometry)
    bad, n = [], max(len(b) for b in BATCHES)
    with H.reconstructor(lib, *geometry, n_streams=n, slots=L.SLOTS, max_pictures=n) as hip:
        for members, want_tuple in BATCHES.items():
            got, tup = run_batch(hip, [kinds[k] for k in members], geometry, "batch %s" % (members,))
            assert tup == want_tuple, (members, tup)
            bad += got
        if "scaled P" in kinds:
            # beside a B picture the scaled P picture goes through k_mc_sort_scaled (the two-list, weighted instance), beside an I
            # picture through the dense scaled intra kernel
            for members, sort, intra in ((("scaled P", "B implicit"), "scaled", "sparse_scaled"), (("scaled P", "I"), "scaled_p", "dense_scaled"),
                                         (("P weighted", "scaled P", "B weighted"), "scaled", "sparse_scaled")):
                got, tup = run_batch(hip, [kinds[k] for k in members], geometry, "batch %s" % (members,))
                assert (tup[0], tup[3]) == (sort, intra), (members, tup)
                bad += got
        if "Cr P" in kinds:
            for members in (("Cr P", "P"), ("B implicit", "Cr P", "I")):
                got, tup = run_batch(hip, [kinds[k] for k in members], geometry, "batch %s" % (members,))
                assert hip.last_cr_pictures() == 1 and tup[0] == ("scaled" if "B implicit" in members else "scaled_p"), (members, tup)
                bad += got
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("geometry", L.GEOMETRIES, ids=L.IDS)
def test_the_roads_into_a_slot(lib, cases, geometry):
    """up to P264HIP_COMPACT_MAX_MB macroblocks every picture through upload and compact (33 x 32 and 64 x 128, where a thread of
    k_expand_compact owns 2 and 8 macroblocks: packed and commit as well); above it through upload, packed and commit, and
    p264hip_upload_compact refuses a block whose header claims the picture - the slot and the frame are as they were afterwards"""
    kinds, sw = cases(geometry), L.switches(geometry)
    roads = ("upload", "packed", "commit") if not sw["compact"] else H.ROADS if geometry in ((33, 32), (64, 128)) else ("upload", "compact")
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=1, slots=L.SLOTS, max_pictures=1) as hip:
        for k, (st, want) in kinds.items():
            H.load_frames(hip, 0, st.frames)
            blank = [np.zeros((geometry[1] * 16 >> (i > 0), geometry[0] * 16 >> (i > 0)), np.uint8) for i in range(3)]
            for road in roads:
                hip.write_frame(0, L.DST, *blank)
                H.put(hip, lib, 0, st.pic, road)
                hip.reconstruct([0], [0])
                bad += same(hip.read_frame(0, L.DST), want, "%s (%s)" % (st.name, road), st.pic)
            hip.sync()
            if not sw["compact"] and k in ("P", "B implicit"):
                with pytest.raises(P264Error):
                    hip.pack_compact(st.pic, lib)
                block = L.consistent_header(st.pic)               # (consistent for 8256 macroblocks: the limit alone refuses it)
                with pytest.raises(P264Error):
                    hip.upload_compact(0, st.pic, block)
                bad += same(hip.read_frame(0, L.DST), want, "%s (the frame after the refused compact upload)" % st.name, st.pic)
                hip.write_frame(0, L.DST, *blank)
                hip.reconstruct([0], [0])                              # the slot still holds the picture the last road put there
                bad += same(hip.read_frame(0, L.DST), want, "%s (after the refused compact upload)" % st.name, st.pic)
                hip.sync()
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("geometry", L.HIGH_GEOMETRIES, ids=L.IDS)
@pytest.mark.parametrize("road", ["upload", "compact"])
def test_high_profile_pictures(lib, oracle, geometry, road):
    """the five pictures of edge_geometry_stim.picture_set, batched as tests/test_gpu_edge_geometry.py batches them: one by one through
    submit, flat and scaled apart (k_mc_sort, k_mc_sort_scaled), and the flat P picture beside the scaled I picture: the one batch of
    these pictures that selects k_mc_sort_scaled_p (the set's only scaled P picture is the weighted one)"""
    stims = L.high_set(geometry)
    cases = [(st, L.expected(oracle, st, "%s/high/%d %s" % (L.IDS(geometry), i, st.name))) for i, st in enumerate(stims)]
    flat, scaled = [c for c in cases if not E.is_scaled(c[0])], [c for c in cases if E.is_scaled(c[0])]
    assert len(flat) == 2 and len(scaled) == 3 and E.runs_k_t8x8(flat[0][0]) and int(scaled[2][0].pic.desc.slice_type) == N.SLICE_I
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=3, slots=L.SLOTS, max_pictures=3) as hip:
        if road == "upload":
            for st, want in cases:
                H.load_frames(hip, 0, st.frames)
                hip.submit(0, st.pic)
                assert hip.last_intra_i8() == 1 and hip.last_scaled_pictures() == int(E.is_scaled(st)), st.name
                bad += same(hip.read_frame(0, L.DST), want, st.name, st.pic)
        for what, batch, sort in (("flat", flat, "plain"), ("scaled", scaled, "scaled"), ("flat P beside scaled I", [flat[0], scaled[2]], "scaled_p")):
            for k, (st, _) in enumerate(batch):
                H.load_frames(hip, k, st.frames)
                hip.write_frame(k, L.DST, *[np.zeros((geometry[1] * 16 >> (i > 0), geometry[0] * 16 >> (i > 0)), np.uint8) for i in range(3)])
                H.put(hip, lib, k, st.pic, road)
            hip.reconstruct(list(range(len(batch))), list(range(len(batch))))
            e, tup = plan_of([st for st, _ in batch], geometry)
            check_report(hip, e, what)
            assert tup[0] == sort and tup[3] == ("dense_i8" if what == "flat" else "dense_scaled"), (what, tup)
            for k, (st, want) in enumerate(batch):
                bad += same(hip.read_frame(k, L.DST), want, "%s (%s batch, %s)" % (st.name, what, road), st.pic)
            hip.sync()
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


# ---- T8X8 records and Intra 8x8 macroblocks at every size ------------------------------------------------------------------------------
def fast_case(oracle, geometry, kind):
    st = L.fast_picture(geometry, kind)
    return st, L.expected(oracle, st, "%s/%s" % (L.IDS(geometry), kind))


@pytest.mark.parametrize("kind", L.FAST)
@pytest.mark.parametrize("geometry", L.FAST_GEOMETRIES, ids=L.IDS)
def test_t8x8_and_intra_8x8_alone_and_through_the_roads(lib, oracle, geometry, kind):
    """a P picture with T8X8 records and Intra 8x8 macroblocks, a dense Intra 8x8 picture, a scaled B and a scaled weighted P picture:
    through submit, then through the roads of test_the_roads_into_a_slot (the compact road with M = 2, 4, 6 and 8)"""
    st, want = fast_case(oracle, geometry, kind)
    sw = L.switches(geometry)
    roads = ("upload", "packed", "commit") if not sw["compact"] else H.ROADS if geometry in ((33, 32), (64, 128)) else ("upload", "compact")
    blank = [np.zeros((geometry[1] * 16 >> (i > 0), geometry[0] * 16 >> (i > 0)), np.uint8) for i in range(3)]
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=1, slots=L.SLOTS, max_pictures=1) as hip:
        H.load_frames(hip, 0, st.frames)
        hip.submit(0, st.pic)
        e, tup = plan_of([st], geometry)
        check_report(hip, e, st.name)
        assert e["intra_i8"] == 1 and tup[3] == {"P T8X8 I8": "sparse_i8", "dense I8": "dense_i8"}.get(kind, "sparse_scaled"), (kind, tup)
        assert kind == "dense I8" or tup[0] == {"P T8X8 I8": "plain", "scaled B": "scaled", "scaled weighted P": "scaled"}[kind], (kind, tup)
        assert (e["t8x8_wgs"] > 0) == (kind == "P T8X8 I8"), (kind, e)
        bad += same(hip.read_frame(0, L.DST), want, st.name, st.pic)
        for road in roads:
            hip.write_frame(0, L.DST, *blank)
            H.put(hip, lib, 0, st.pic, road)
            hip.reconstruct([0], [0])
            bad += same(hip.read_frame(0, L.DST), want, "%s (%s)" % (st.name, road), st.pic)
        hip.sync()
    assert not bad, "%d runs differ: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("geometry", L.FAST_GEOMETRIES, ids=L.IDS)
def test_t8x8_and_intra_8x8_in_batches(lib, oracle, geometry):
    """flat and scaled apart, and the flat P picture beside the scaled B picture; one reconstruct call each"""
    kinds = {k: fast_case(oracle, geometry, k) for k in L.FAST}
    L.assert_fast_covered(geometry, {k: v[0] for k, v in kinds.items()})
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=4, slots=L.SLOTS, max_pictures=4) as hip:
        for members, sort, intra in ((("P T8X8 I8", "dense I8"), "plain", "dense_i8"), (("scaled B", "scaled weighted P"), "scaled", "sparse_scaled"),
                                     (("scaled B", "P T8X8 I8"), "scaled", "sparse_scaled"), (L.FAST, "scaled", "dense_scaled")):
            got, tup = run_batch(hip, [kinds[k] for k in members], geometry, "batch %s" % (members,))
            assert (tup[0], tup[3]) == (sort, intra), (members, tup)
            bad += got
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("geometry", L.LIMIT_GEOMETRIES, ids=L.IDS)
def test_limit_vectors_inside_the_picture(lib, oracle, geometry):
    """P and B, unweighted and with explicit weights: windows 2048 samples to the side or 512 up or down, inside the reference"""
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=1, slots=L.SLOTS, max_pictures=1) as hip:
        for st in L.limit_vector_set(geometry):
            L.assert_limit_covered(st)
            twin = L.weighted_twin(st)
            key = "%s/%s" % (L.IDS(geometry), st.name) if st.pic.n_mb > L.IN_TEST_MB else None
            H.load_frames(hip, 0, st.frames)
            for s, want in ((st, L.expected(oracle, st)), (twin, L.expected(oracle, twin, key))):
                hip.submit(0, s.pic)
                check_report(hip, plan_of([s], geometry)[0], s.name)
                bad += same(hip.read_frame(0, L.DST), want, s.name, s.pic)
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


def clear_knobs(monkeypatch):
    import os
    for name in list(os.environ):
        if name.startswith(K + "MC_") or name.startswith(K + "DEBLOCK_") or name in (K + "INTRA_WAVES", K + "BS_FUSED"):
            monkeypatch.delenv(name)


@pytest.mark.parametrize("rb_log2", ["1", "2", "3"])
@pytest.mark.parametrize("geometry", [(3, 512), (1, 161)], ids=L.IDS)
def test_tall_pictures_through_the_loop_filter_s_bands(lib, cases, geometry, rb_log2, monkeypatch):
    """P264AMD_DEBLOCK_RB_LOG2 = 1, 2, 3: at 1 a picture of 512 rows has 256 bands, MAX_BANDS exactly.  The five kinds in one call;
    at 1 also sixteen pictures (the five and clones of them) served by ONE workgroup: every entry of progress[16][256]"""
    clear_knobs(monkeypatch)
    monkeypatch.setenv(K + "DEBLOCK_RB_LOG2", rb_log2)                       # (the knobs are read when the context is created)
    kinds = cases(geometry)
    members = [kinds[k] for k in L.MAIN]
    with H.reconstructor(lib, *geometry, n_streams=5, slots=L.SLOTS, max_pictures=5) as hip:
        bad, _ = run_batch(hip, members, geometry, "RB_LOG2 %s" % rb_log2)
        assert hip.last_launch()["deblock_rb_log2"] == int(rb_log2)
    if rb_log2 == "1":
        monkeypatch.setenv(K + "DEBLOCK_PICS_PER_WG", "16")
        with H.reconstructor(lib, *geometry, n_streams=16, slots=L.SLOTS, max_pictures=16) as hip:
            for s in range(16):
                H.load_frames(hip, s, members[s % 5][0].frames)
            hip.upload(0, [st.pic for st, _ in members])
            for s in range(5, 16):
                hip.clone_picture(s, s % 5)
            hip.reconstruct(list(range(16)), list(range(16)))
            li = hip.last_launch()
            assert li["deblock_pics_per_wg"] == 16 and li["deblock_rb_log2"] == 1 and li["pictures"] == 16, li
            for s in range(16):
                st, want = members[s % 5]
                bad += same(hip.read_frame(s, L.DST), want, "%s (entry %d of 16 in one workgroup)" % (st.name, s), st.pic)
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("waves", ["1", "4", "16"])
@pytest.mark.parametrize("geometry", [(1, 161), (65, 81), (3, 512)], ids=L.IDS)
def test_intra_wavefront_counts(lib, oracle, cases, geometry, waves, monkeypatch):
    """P264AMD_INTRA_WAVES = 1, 4, 16 where use_free is off: all six instances - sparse and dense, plain, Intra 8x8 and scaled.  One wavefront walks every band in order; sixteen hand over between all of them"""
    clear_knobs(monkeypatch)
    monkeypatch.setenv(K + "INTRA_WAVES", waves)
    kinds = dict(cases(geometry))
    assert not L.switches(geometry)["use_free"]
    batches = [("P",), ("B implicit",), ("P", "I")]
    if geometry in L.HIGH_GEOMETRIES:
        # the High-profile set: P flat (sparse_i8), beside the dense I (dense_i8), scaled B (sparse_scaled), beside the scaled I (dense_scaled)
        hs = L.high_set(geometry)
        kinds.update({"high %d" % i: (st, L.expected(oracle, st, "%s/high/%d %s" % (L.IDS(geometry), i, st.name))) for i, st in enumerate(hs)})
        batches += [("high 0",), ("high 0", "high 1"), ("high 2",), ("high 2", "high 4")]
    else:
        kinds.update({k: fast_case(oracle, geometry, k) for k in L.FAST})
        batches += [("P T8X8 I8",), ("P T8X8 I8", "dense I8"), ("scaled B",), ("scaled B", "dense I8")]
        batches += [(k,) for k in ("scaled P", "Cr P") if k in kinds] + ([("scaled P", "I")] if "scaled P" in kinds else [])
    intras = {plan_of([kinds[k][0] for k in m], geometry)[1][3] for m in batches}
    assert intras == {"sparse", "dense", "sparse_i8", "dense_i8", "sparse_scaled", "dense_scaled"}, intras
    bad = []
    with H.reconstructor(lib, *geometry, n_streams=2, slots=L.SLOTS, max_pictures=2) as hip:
        for members in batches:
            got, _ = run_batch(hip, [kinds[k] for k in members], geometry, "INTRA_WAVES %s, %s" % (waves, members))
            assert hip.last_launch()["intra_waves"] == int(waves), hip.last_launch()
            bad += got
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


# ---- frames out at the limits ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_frames(lib):
    """far_frames(geometry) -> (context, {(0, 0): planes}): one frame of random samples"""
    open_ = {}

    def of(geometry):
        if geometry not in open_:
            hip = H.HipReconstructor(*geometry, lib=lib, n_streams=1, slots=1, max_pictures=1)
            hip.write_frame(0, 0, *seam_fuzz.random_frame(np.random.default_rng([2660, geometry[0]]), *geometry))
            open_[geometry] = (hip, {(0, 0): hip.read_frame(0, 0)})
        return open_[geometry]
    yield of
    for hip, _ in open_.values():
        hip.close()


def far_windows(geometry):
    """the whole frame, and a window that ends at the last column / row"""
    w, h = geometry[0] * 16, geometry[1] * 16
    return [(0, 0, w, h), (w - 752, 2, 752, h - 2) if w > h else (2, h - 592, w - 2, 592)]


@pytest.mark.parametrize("fmt", ["i420", "nv12", "rgb24", "rgbp"])
@pytest.mark.parametrize("geometry", L.LIMIT_GEOMETRIES, ids=L.IDS)
def test_frames_out_at_the_far_end(far_frames, geometry, fmt):
    from tests.test_gpu_export import run as run_export
    hip, planes = far_frames(geometry)
    for n, crop in enumerate(far_windows(geometry)):
        pitch = 0 if n == 0 else X.tight_pitch(fmt, crop[2]) + 16
        matrix, full = ("bt709", True) if n and fmt.startswith("rgb") else ("bt601", False)
        got, want = run_export(hip, planes, [0], [0], fmt, crop, matrix, full, pitch, 0, 4 * n)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s window %s: %d bytes differ, the first at %d" % (fmt, crop, bad.size, bad[0])


@pytest.mark.parametrize("fmt", ["i420", "nv12", "rgb24", "rgbp"])
@pytest.mark.parametrize("geometry", L.LIMIT_GEOMETRIES, ids=L.IDS)
def test_resized_from_the_far_end(far_frames, geometry, fmt):
    """both filters from a window at the far end of the frame: on 2047 x 2 columns 32000 .. 32751 to 94 x 4 (8:1) and - antialiased -
    to 48 x 2 (16:1; an output size is even, so 47 x 2 is not one); on 3 x 512 rows 7600 .. 8191 reduced 8:1.  The whole destination prefilled and compared"""
    from tests.test_gpu_resize import run as run_bilinear
    from tests.test_gpu_resize_aa import run as run_aa
    hip, planes = far_frames(geometry)
    if geometry[0] > geometry[1]:
        crop, sizes = (32000, 0, 752, 32), [(run_bilinear, (94, 4)), (run_aa, (94, 4)), (run_aa, (48, 2))]
    else:
        crop, sizes = (0, 7600, 48, 592), [(run_bilinear, (6, 74)), (run_aa, (6, 74))]
    for run, size in sizes:
        got, want = run(hip, planes, [0], [0], fmt, crop, size, "u8", None, None, "bt601", False, 0, 0, 0)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "%s %s window %s to %s: %d bytes differ, the first at %d" % (run.__module__, fmt, crop, size, bad.size, bad[0])


# ---- what p264hip_create refuses, and the extremes it accepts ------------------------------------------------------------------------
def test_create_refuses_what_no_entry_can_hold(lib):
    c = L.constants()
    max_w, max_h = (1 << c["MCE_COL_BITS"]) - 1, c["MAX_MB_ROWS"]
    assert (max_w, max_h) == (2047, 512)
    for w, h in ((max_w + 1, 1), (1, max_h + 1)):
        ctx = C.c_void_p()
        assert lib.p264hip_create(C.byref(ctx), 0, w, h, 1, 2, 1) == -1 and not ctx.value          # P264HIP_EINVAL
        assert b"bad argument" in lib.p264hip_last_error()
    # (this check comes before any allocation: 17 slots of 402 MB are never asked for)
    ctx = C.c_void_p()
    assert lib.p264hip_create(C.byref(ctx), 0, max_w, max_h, 1, 17, 1) == -1 and not ctx.value
    assert b"frame store of one stream exceeds" in lib.p264hip_last_error()


@pytest.mark.parametrize("geometry", [(2047, 1), (1, 512)], ids=L.IDS)
def test_create_accepts_the_extremes(lib, oracle, geometry):
    st = L.main_picture(geometry, "P")
    want = L.expected(oracle, st)
    with H.reconstructor(lib, *geometry, n_streams=1, slots=L.SLOTS, max_pictures=1) as hip:
        H.load_frames(hip, 0, st.frames)
        hip.submit(0, st.pic)
        H.compare(hip.read_frame(0, L.DST), want, st.name, st.pic)
