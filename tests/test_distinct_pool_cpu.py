"""CPU check of the pools of distinct sources (tests/distinct_pool.py) that the GPU tests test_gpu_distinct_shapes.py and
test_gpu_distinct_bench.py decode: the sources really differ in what a picture carries, and no k_deblock workgroup of any shape
those tests run holds two pictures of one source.  The High-profile pools are pinned to committed hashes
(tests/golden/high_pool.json): here, where no GPU waits, tests/scaling_checker.py decodes every source again - the hashes are the
standard's, no macroblock of any picture is without a defined result, and the pictures hold what the pools are there for."""
import hashlib
from collections import Counter

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import distinct_pool, scaling_checker, stream_args as shapes
from tests.conftest import frame_sha256

POOLS = {"p": (distinct_pool.POOL_P, 8, 17), "b": (distinct_pool.POOL_B, 7, 17), "wp": (distinct_pool.POOL_WP, 7, 17),
         "bench": (distinct_pool.POOL_BENCH, 4, 9), "cfg4": (distinct_pool.POOL_CFG4, 7, 9),
         "high": (distinct_pool.POOL_HIGH, 7, 17), "scaled": (distinct_pool.POOL_SCALED, 7, 18),
         "scaled_plain": (distinct_pool.POOL_SCALED_PLAIN, 7, 18)}
N_CU = 256                               # an MI355X (the GPU tests assert the shapes they get)
# (streams, pictures per k_deblock workgroup) of every batch the GPU tests run
BATCHES = {name: [(shapes.DISTINCT_STREAMS, int(pw)) for _, pw, _ in shapes.LAUNCH_SHAPES] + [(shapes.DISTINCT_STREAMS, int(pw)) for pw in shapes.ODD] +
           [(shapes.DISTINCT_STREAMS, int(pw)) for _, pw, _ in shapes.WAVES] + [(shapes.DISTINCT_STREAMS, 1)]
           for name in ("p", "b", "wp", "high", "scaled", "scaled_plain")}
BATCHES["bench"] = [(8 * N_CU, 8)]
BATCHES["cfg4"] = [(4 * N_CU, 4)]


@pytest.fixture(scope="module")
def parsed(lib):
    return {name: distinct_pool.Pool(lib, specs, n) for name, (specs, n, _) in POOLS.items()}


def slice_qp(pic):
    """the QP of every non-PCM macroblock, if they all have one (no mb_qp_delta), else None"""
    rec = pic.mb_records()
    qps = set(rec["qp"][rec["mb_type"] != N.MB_IPCM].tolist())
    return qps.pop() if len(qps) == 1 else None


@pytest.mark.parametrize("name", list(POOLS))
def test_the_sources_differ_in_every_per_picture_parameter(parsed, name):
    pool = parsed[name]
    assert pool.K >= POOLS[name][2] and len(set(POOLS[name][0])) == pool.K
    first_p = [next(p for p in s.pics if p.desc.slice_type == N.SLICE_P) for s in pool.sources]
    cqo = [p.desc.chroma_qp_offset for p in first_p]
    assert min(cqo) < 0 < max(cqo), cqo
    offs = [(p.desc.alpha_c0_offset, p.desc.beta_offset) for p in first_p]
    assert len(set(offs)) >= 4, offs
    nodeblock = [all(not p.desc.deblock for p in s.pics) for s in pool.sources]
    assert sum(nodeblock) == 1 and all(all(p.desc.deblock for p in s.pics) for s, off in zip(pool.sources, nodeblock) if not off)
    assert sum(slice_qp(p) is None for p in first_p) >= 1, "no source with a QP per macroblock"
    assert len({max(p.desc.n_ref for p in s.pics) for s in pool.sources}) >= 2, "every source has the same number of references"
    # two sources with one slice QP and different loop-filter offsets: the octet's cache of expanded alpha / beta is keyed by QP
    by_qp = {}
    for p in first_p:
        if slice_qp(p) is not None and p.desc.deblock:
            by_qp.setdefault(slice_qp(p), set()).add((p.desc.alpha_c0_offset, p.desc.beta_offset))
    assert any(len(v) >= 2 for v in by_qp.values()), by_qp


@pytest.mark.parametrize("name", list(POOLS))
def test_the_kinds_of_pictures_of_each_pool(parsed, name):
    pool = parsed[name]
    steps = [Counter(p.desc.slice_type for p in pool.step_pictures(t)) for t in range(pool.n_pictures)]
    assert set(steps[0]) == {N.SLICE_I}
    wp = [any(p.desc.explicit_wp for p in s.pics) for s in pool.sources]
    if name in ("p", "bench"):
        assert all(set(c) <= {N.SLICE_P, N.SLICE_I} for c in steps) and sum(set(c) == {N.SLICE_P} for c in steps) >= 3
        assert not any(wp)
        return
    specs = POOLS[name][0]
    assert all(any(p.desc.slice_type == N.SLICE_B for p in s.pics) for s in pool.sources)
    assert {N.SLICE_P} in [set(c) for c in steps] and {N.SLICE_B} in [set(c) for c in steps]
    assert sum(set(c) == {N.SLICE_P, N.SLICE_B} for c in steps) >= 3, "no steps that mix P and B pictures"
    assert Counter("--bframes 1 " in s for s in specs)[True] >= 1
    assert Counter("--bframes 2 " in s or s in distinct_pool.synth_cases.ORACLE_CASES for s in specs)[True] > pool.K // 2
    implicit = {p.desc.weighted_bipred for s in pool.sources for p in s.pics if p.desc.slice_type == N.SLICE_B}
    assert implicit == {0, 1}
    for opt in ("--cabac", "--temporal"):            # (the entropy coder and the direct mode leave no trace in the descriptor)
        with_opt = [opt in (distinct_pool.synth_cases.ORACLE_CASES.get(s, s)) for s in specs]
        assert 0 < sum(with_opt) < pool.K, opt
    if name in ("wp", "scaled"):
        assert sum(wp) == 1
        kinds = {p.desc.slice_type for s, w in zip(pool.sources, wp) if w for p in s.pics if p.desc.explicit_wp}
        assert kinds == {N.SLICE_P, N.SLICE_B}
    else:
        assert not any(wp)


@pytest.mark.parametrize("name", list(POOLS))
def test_no_deblocking_workgroup_holds_two_pictures_of_one_source(parsed, name):
    pool = parsed[name]
    for S, per_wg in BATCHES[name]:
        assert per_wg < pool.K
        order = pool.order(S, 1)
        assert sorted(order) == list(range(S)) and order != list(range(S))
        for w, srcs in enumerate(pool.workgroups(S, per_wg)):
            assert len(set(srcs)) == len(srcs), "S %d, %d per workgroup: workgroup %d holds sources %s" % (S, per_wg, w, srcs)
        assert len({j % pool.K for j in range(S)}) == pool.K
    assert pool.slots == max(s.slots for s in pool.sources)


# ---- the High-profile pools ----------------------------------------------------------------------------------------------------
HIGH_POOLS = ("high", "scaled", "scaled_plain")


@pytest.fixture(scope="module")
def standard(parsed):
    """{spec: per picture ([y, u, v] by scaling_checker.SpecRecon, the level blocks that feed a value out of range, the Census of
    its blocks, the lines the loop filter's 8x8 edge mask kept unchanged)} of every source of the two pools, decoded once"""
    out = {}
    for name in HIGH_POOLS:
        for s in parsed[name].sources:
            if s.spec not in out:
                masked = []
                frames = distinct_pool.spec_frames(s.pics, s.slots, masked)
                seen = [scaling_checker.Census() for _ in s.pics]
                out[s.spec] = [(f, scaling_checker.census(p, c)[1], c, k) for f, p, c, k in zip(frames, s.pics, seen, masked)]
    return out


def flags(pic, bit):
    return int(((pic.mb_records()["intra_modes"] & bit) != 0).sum())


def table(pic):
    return bytes(pic.desc.scaling4x4) + bytes(pic.desc.scaling8x8) if int(pic.desc.scaling_lists) else None


def test_the_committed_hashes_are_what_the_standard_gives(parsed, standard):
    """tests/golden/high_pool.json against the checker, and the condition under which a byte-exact comparison means something: no
    macroblock of any picture of any source leaves the range in which H.264 defines the result - none is excluded anywhere"""
    assert sorted(standard) == sorted(distinct_pool.HIGH_SPECS)
    for name in HIGH_POOLS:
        for s in parsed[name].sources:
            digest, hashes = distinct_pool.high_golden(s.spec)
            data = distinct_pool.read_stream(s.spec)
            assert hashlib.sha256(data).hexdigest() == digest, s.spec
            assert len(hashes) == len(s.pics) == len(standard[s.spec])
            for i, (frame, out_of_range, _, _) in enumerate(standard[s.spec]):
                assert not out_of_range, "%s picture %d: %d level blocks feed a value out of range: %s" % (s.spec, i, len(out_of_range), sorted(out_of_range, key=str)[:3])
                assert frame_sha256(*frame) == hashes[i], "%s picture %d: the committed hash is not the checker's picture" % (s.spec, i)


def test_what_the_high_profile_pools_are_for(parsed, standard):
    """`high`: in every step behind the IDR every source's picture has macroblocks with the 8x8 transform and at least half have
    Intra 8x8 macroblocks - k_t8x8 and the _i8 intra instances have work in every picture; no lists anywhere.  `scaled`: in every
    step pictures with lists stand beside flat ones with and without 8x8 blocks, the scaled ones reach all eight lists at weights
    other than 16 (the four intra lists in the IDR step) and carry at least four different tables"""
    high, scaled = parsed["high"], parsed["scaled"]
    assert not any(int(p.desc.scaling_lists) for s in high.sources for p in s.pics)
    for t in range(1, high.n_pictures):
        pics = high.step_pictures(t)
        assert all(p.desc.slice_type != N.SLICE_I and flags(p, N.MB_T8X8) > 0 for p in pics), t
        assert 2 * sum(flags(p, N.MB_I8X8) > 0 for p in pics) >= high.K, t
    # the loop filter's edge mask matters: in every step, in more than half of the pool's pictures (those without the filter or
    # without the 8x8 transform counted), leaving luma edges 1 and 3 of macroblocks with the 8x8 transform alone changes samples -
    # whatever the pictures per k_deblock workgroup, most workgroups hold pictures that show another picture's edge info
    for pool in (high, scaled, parsed["scaled_plain"]):
        for t in range(pool.n_pictures):
            masked = [standard[s.spec][t][3] for s in pool.sources]
            assert 2 * sum(k > 0 for k in masked) > pool.K, (t, masked)
    is_scaled = [bool(int(s.pics[0].desc.scaling_lists)) for s in scaled.sources]
    assert all(bool(int(p.desc.scaling_lists)) == sc for s, sc in zip(scaled.sources, is_scaled) for p in s.pics)
    flat = [s for s, sc in zip(scaled.sources, is_scaled) if not sc]
    assert sum(is_scaled) >= 8 and sum(s.spec in distinct_pool.POOL_HIGH for s in flat) >= scaled.K // 2 - 1
    assert sum(not any(int(p.desc.transform_8x8) for p in s.pics) for s in flat) == 1, "one flat source without any 8x8 block"
    where = Counter(w for s in scaled.sources for w in ("sps", "pps", "both") if "--cqm-where %s " % w in s.spec + " ")
    assert all(where[w] >= 1 for w in ("sps", "pps", "both")), where
    # no workgroup-sized run of entries is all scaled or all flat: neighbours in a batch differ in the table they take
    assert all(is_scaled[j] != is_scaled[(j + 1) % scaled.K] for j in range(scaled.K) if j != scaled.K - 1)
    for t in range(scaled.n_pictures):
        pics = scaled.step_pictures(t)
        with_lists = [p for p, sc in zip(pics, is_scaled) if sc]
        assert 0 < len(with_lists) < len(pics)
        assert len({table(p) for p in with_lists}) >= 4, t
        reached = Counter()
        for s, sc in zip(scaled.sources, is_scaled):
            if sc:
                reached.update(standard[s.spec][t][2].lists)
        lists = range(8) if t else (scaling_checker.INTRA_Y, scaling_checker.INTRA_CB, scaling_checker.INTRA_CR, scaling_checker.INTRA_Y8)
        assert all(reached[n] > 0 for n in lists), (t, dict(reached))
        if t:
            assert any(flags(p, N.MB_T8X8) for p, sc in zip(pics, is_scaled) if not sc), "step %d: no flat picture whose 8x8 blocks k_scaled_inter owns" % t


def test_the_scaled_pools_take_every_scaled_sort(parsed):
    """`scaled` has an explicit-weight picture in every step behind the IDR: always k_mc_sort_scaled and k_mc_wp.  `scaled_plain` is the
    same pool but for that source, which keeps its lists and loses its weights: its step of P pictures takes k_mc_sort_scaled_p
    and k_mc, its steps with B pictures k_mc_sort_scaled, k_mc and k_mc_second - by launch_inter's rule over the kinds of the
    batch's pictures (p264hip.hip), which distinct_pool.expected_inter_instances restates"""
    scaled, plain = parsed["scaled"], parsed["scaled_plain"]
    differ = [k for k in range(scaled.K) if scaled.sources[k].spec != plain.sources[k].spec]
    assert len(differ) == 1 and any(p.desc.explicit_wp for p in scaled.sources[differ[0]].pics)
    assert not any(p.desc.explicit_wp for s in plain.sources for p in s.pics)
    assert [[int(p.desc.scaling_lists) for p in s.pics] for s in plain.sources] == [[int(p.desc.scaling_lists) for p in s.pics] for s in scaled.sources]
    want = distinct_pool.expected_inter_instances
    assert want(scaled.step_pictures(0)) == want(plain.step_pictures(0)) == ()
    for t in range(1, scaled.n_pictures):
        assert want(scaled.step_pictures(t))[:2] == ("k_mc_sort_scaled", "k_mc_wp"), t
    kinds = [want(plain.step_pictures(t)) for t in range(1, plain.n_pictures)]
    assert kinds[0] == ("k_mc_sort_scaled_p", "k_mc") and set(kinds[1:]) == {("k_mc_sort_scaled", "k_mc", "k_mc_second")}, kinds


def test_a_source_says_where_a_picture_differs(parsed, standard):
    """Source.check on plain arrays: the expected picture passes by its committed hash; with one sample changed the checker's own
    picture is computed and the message names plane, position and both values"""
    s = parsed["scaled"].sources[0]
    s.expect()
    assert s.frames is None
    want = standard[s.spec][3][0]
    s.check(3, [a.copy() for a in want], "unchanged")
    assert s.frames is None                                  # (no checker run for a picture that matches)
    got = [a.copy() for a in want]
    got[1][5, 7] ^= 0x10
    with pytest.raises(AssertionError) as e:
        s.check(3, got, "entry 4 (source 0) stream 9")
    text = str(e.value)
    assert "entry 4 (source 0) stream 9" in text and s.spec in text and "picture 3" in text
    assert "plane 1: 1 samples, first (y=5,x=7) got %d want %d" % (got[1][5, 7], want[1][5, 7]) in text, text
    assert "committed hash too" not in text
    assert all(np.array_equal(a, b) for f, (w, _, _, _) in zip(s.frames, standard[s.spec]) for a, b in zip(f, w))
