"""Every kind of picture through every kernel set a batch can select.  p264hip_reconstruct picks one kernel instance per stage for
ALL pictures of a call (launch_plan.h), so a picture decodes through different code depending on what shares its call.
tests/batch_kinds.py holds a table of picture kinds (the seven of tests/test_gpu_batch_composition.py, and P / B / I pictures with
the 8x8 transform, Intra 8x8, scaling lists, a Cr QP offset of its own, I_PCM, a list 0 that holds a frame twice, and all of it at
once) and cover(): subsets of up to four kinds that reach every (kind, instance tuple) cell such subsets can reach, and every tuple
at all (tests/test_batch_kinds_cpu.py asserts both).  Here every subset of the cover is one reconstruct call; every member must be,
byte for byte, the picture the text of H.264 gives for it alone (cr_offset_checker.TwoChains over scaling_checker.SpecRecon, which
tests/test_batch_kinds_cpu.py ties to the oracle), and the launch must report what the subset's tuple implies.  Then the subsets
with a dup-list or an everything-at-once kind through the compact road, and 600 small pictures of every kind in one call."""
import numpy as np
import pytest

from tests import batch_kinds as BK
from tests import hip_harness as H
from tests.batch_kinds import LARGE_H, LARGE_W

pytestmark = pytest.mark.gpu

PARTS = 8                          # slices of the cover, so that no test runs more than a few seconds
N_LARGE = 600
FRAGILE = set(BK.DUP) | {"P_all", "B_all"}       # the kinds no earlier stimulus module draws beside High-profile pictures


@pytest.fixture(scope="module")
def kinds():
    """{name: (stimulus, [y, u, v] by the standard)}, computed once"""
    return {name: (st, BK.expected(st)) for name, st in BK.pictures().items()}


@pytest.fixture(scope="module")
def large_kinds():
    return {name: (st, BK.expected(st)) for name, st in BK.pictures(1405, LARGE_W, LARGE_H).items()}


@pytest.fixture(scope="module")
def pool(lib, kinds):
    """one context, one stream per kind with the kind's reference frames written once"""
    with H.reconstructor(lib, BK.W, BK.H, n_streams=len(BK.NAMES), slots=BK.SLOTS, max_pictures=len(BK.NAMES)) as hip:
        for s, name in enumerate(BK.NAMES):
            H.load_frames(hip, s, kinds[name][0].frames)
        yield hip


def implied(members, flags, n_mb):
    """what the launch must report for a batch of these kinds: the plan's rules (tests/batch_kinds.py) over the members' flags"""
    return BK.plan_rules(BK.union(flags[m] for m in members), len(members), None, n_mb)


def check_report(hip, e, what):
    li = hip.last_launch()
    assert (li["edge_info_fused"] > 0) == (e["edge"] == "fused") and li["edge_info_fused"] == e["edge_info_fused"], "%s: edge_info_fused %d" % (what, li["edge_info_fused"])
    assert (hip.last_t8x8_wgs() > 0) == (e["residual"] == "t8x8") and hip.last_t8x8_wgs() == e["t8x8_wgs"], "%s: t8x8_wgs %d" % (what, hip.last_t8x8_wgs())
    assert hip.last_scaled_pictures() == e["scaled_pictures"] and hip.last_cr_pictures() == e["cr_pictures"], "%s: scaled %d, cr %d" % (
        what, hip.last_scaled_pictures(), hip.last_cr_pictures())
    assert hip.last_intra_i8() == e["intra_i8"] and li["pictures"] == e["pictures"], "%s: intra_i8 %d, pictures %d" % (what, hip.last_intra_i8(), li["pictures"])
    return li


def run(hip, lib, kinds, members, road="upload"):
    """the kinds `members` in one call, each on its own stream: the launch's report checked, the differences returned"""
    blank = [np.zeros_like(a) for a in kinds[members[0]][1]]
    streams = [BK.NAMES.index(m) for m in members]
    for s in streams:
        hip.write_frame(s, BK.DST, *blank)
    if road == "upload":
        hip.upload(0, [kinds[m][0].pic for m in members])
    else:
        for k, m in enumerate(members):
            H.put(hip, lib, k, kinds[m][0].pic, road)
    hip.reconstruct(list(range(len(members))), streams)
    t = BK.tuple_of(members)
    what = "subset %s (%s), tuple %s" % (list(members), road, dict(zip(BK.TUPLE, t)))
    check_report(hip, implied(members, BK.kind_flags(), BK.W * BK.H), what)
    bad = []
    for m, s in zip(members, streams):
        bad += H.differences(hip.read_frame(s, BK.DST), kinds[m][1], "%s in %s" % (m, what), kinds[m][0].pic)
    hip.sync()
    return bad


@pytest.mark.parametrize("part", range(PARTS))
def test_every_kind_through_every_plan(lib, kinds, pool, part):
    cover = BK.cover()
    mine = cover[part::PARTS]
    assert mine and sum(len(cover[p::PARTS]) for p in range(PARTS)) == len(cover)
    bad = []
    for members in mine:
        bad += run(pool, lib, kinds, members)
    assert not bad, "%d pictures of %d subsets differ: %s" % (len(bad), len(mine), bad[:4])


@pytest.mark.parametrize("part", range(2))
def test_through_the_compact_road(lib, kinds, pool, part):
    fragile = [m for m in BK.cover() if len(m) >= 2 and FRAGILE & set(m)]
    assert len(fragile) >= 20 and all(any(k in m for m in fragile) for k in FRAGILE)
    bad = []
    for members in fragile[part::2]:
        bad += run(pool, lib, kinds, members, "compact")
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:4])


@pytest.mark.parametrize("per_wg", [None, "7"])
def test_a_large_batch_of_every_kind(lib, large_kinds, per_wg, monkeypatch):
    """more pictures than 2 x compute units in one call: intra_waves drops to a quarter, the loop filter packs several pictures per
    workgroup (7: odd, in groups, the last workgroup partly empty).  Entry j decodes kind j % K on stream order[j], a shuffled
    permutation: any K consecutive entries hold K different kinds, and an entry's index is not its stream."""
    if per_wg:
        monkeypatch.setenv("P264AMD_DEBLOCK_PICS_PER_WG", per_wg)             # (the knobs are read when the context is created)
    K, n, n_mb = len(BK.NAMES), N_LARGE, LARGE_W * LARGE_H
    order = [int(x) for x in np.random.default_rng(601).permutation(n)]
    ids = [j % K for j in range(n)]
    blank = [np.zeros_like(a) for a in large_kinds[BK.NAMES[0]][1]]
    flags = {name: BK.flags_of(st.pic) for name, (st, _) in large_kinds.items()}
    assert flags == BK.kind_flags()
    with H.reconstructor(lib, LARGE_W, LARGE_H, n_streams=n, slots=BK.SLOTS, max_pictures=K) as hip:
        for j, s in enumerate(order):
            H.load_frames(hip, s, large_kinds[BK.NAMES[ids[j]]][0].frames)
            hip.write_frame(s, BK.DST, *blank)
        hip.upload(0, [large_kinds[name][0].pic for name in BK.NAMES])
        # every kind once: the small batch's shapes
        hip.reconstruct(ids[:K], order[:K])
        small = check_report(hip, implied(BK.NAMES, flags, n_mb), "every kind once")
        hip.reconstruct(ids, order)
        big = check_report(hip, implied([BK.NAMES[k] for k in ids], flags, n_mb), "%d pictures" % n)
        bad = []
        for j, s in enumerate(order):
            name = BK.NAMES[ids[j]]
            bad += H.differences(hip.read_frame(s, BK.DST), large_kinds[name][1], "entry %d (%s) on stream %d" % (j, name, s), large_kinds[name][0].pic)
    assert n > 2 * big["compute_units"], "the batch does not reach the large-batch shapes on this device (%d CUs)" % big["compute_units"]
    assert big["intra_waves"] < small["intra_waves"], (small, big)
    assert big["deblock_pics_per_wg"] > 1 and big["edge_info_fused"] == 0, big
    if per_wg:
        assert big["deblock_pics_per_wg"] == 7 and n % 7 and big["deblock_wgs"] == (n + 6) // 7, big
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), n, bad[:4])
