"""CPU check of the pools of distinct sources (tests/distinct_pool.py) that the GPU tests test_gpu_distinct_shapes.py and
test_gpu_distinct_bench.py decode: the sources really differ in what a picture carries, and no k_deblock workgroup of any shape
those tests run holds two pictures of one source."""
from collections import Counter

import pytest

from p264decoder_amd import _native as N
from tests import distinct_pool, stream_args as shapes

POOLS = {"p": (distinct_pool.POOL_P, 8, 17), "b": (distinct_pool.POOL_B, 7, 17), "wp": (distinct_pool.POOL_WP, 7, 17),
         "bench": (distinct_pool.POOL_BENCH, 4, 9), "cfg4": (distinct_pool.POOL_CFG4, 7, 9)}
N_CU = 256                               # an MI355X (the GPU tests assert the shapes they get)
# (streams, pictures per k_deblock workgroup) of every batch the GPU tests run
BATCHES = {name: [(shapes.DISTINCT_STREAMS, int(pw)) for _, pw, _ in shapes.LAUNCH_SHAPES] + [(shapes.DISTINCT_STREAMS, int(pw)) for pw in shapes.ODD] +
           [(shapes.DISTINCT_STREAMS, int(pw)) for _, pw, _ in shapes.WAVES] + [(shapes.DISTINCT_STREAMS, 1)]
           for name in ("p", "b", "wp")}
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
    if name == "wp":
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
