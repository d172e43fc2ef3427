"""The work lists of the motion-compensation stage at their extremes on the MI355X: the directed pictures of tests/worklist_stim.py
(what each asks of k_mc_sort* and of the chunk walks of k_mc / k_mc_wp / k_mc_second is proved in tests/test_worklist_cpu.py) one by
one and in batches, all three planes byte for byte against tests/spec_recon.py - the standard-only model, computed once per module.
The lists are never read back: a key's segment one chunk short, a class byte in the wrong place, a lost MCE_KEEP entry or a list
that outgrows its room shows in the picture - or, the per-picture scratch lying back to back, in the NEXT picture of the batch.  So
the batches put an ordinary picture behind every extreme one, and every order also runs with the extreme picture last.

All batches of one geometry and knob pair run in one context of seven streams (hip_harness.run_batches); the orders with fewer
pictures are filled up to seven with further ordinary pictures, in front where the extreme picture has to be last.  The knobs:
P264AMD_MC_BAND_LOG2 0 (32 x 4: four bands; 8 x 32: 32 bands of one row, MC_MAX_BANDS), unset (one band of 16 rows / two) and 9 (one
band), crossed with P264AMD_MC_WGS_PER_PIC 4 (few workgroups over many part-filled chunks) and 200 (workgroups without a chunk)."""
import pytest

from p264decoder_amd import _native as N
from tests import spec_recon
from tests import worklist_stim as WS
from tests.hip_harness import expect, run_batches, submit_each

pytestmark = pytest.mark.gpu
SLOTS = WS.SLOTS
N_BATCH = 7
BAND_KNOBS = ("0", None, "9")
WGS_KNOBS = ("4", "200")


@pytest.fixture(scope="module")
def cases():
    """{name: (stim, [y, u, v] by the standard)}: the directed pictures and, per geometry, five ordinary P and two ordinary B pictures"""
    stims = dict(WS.all_stims())
    for geom in (WS.WIDE, WS.DEEP):
        for b_picture, n in ((False, 5), (True, 2)):
            for k in range(n):
                st = WS.ordinary(geom, b_picture, k)
                stims[st.name] = st
    return {name: (st, expect(st, spec_recon.SpecRecon, SLOTS)) for name, st in stims.items()}


def orders(geom):
    """[(what, [names])]: the batches of a geometry, each of N_BATCH distinct pictures"""
    g = "%dx%d" % geom
    P = ["ordinary P %s #%d" % (g, k) for k in range(5)]
    B = ["ordinary B %s #%d" % (g, k) for k in range(2)]
    empty, one_key, all_skip, mid = "empty " + g, "one_key " + g, "all_skip " + g, "single_mid " + g
    out = []
    if geom == WS.WIDE:
        for each in ("ym_each_key", "yq_each_key"):
            out.append(("p", [each, P[0], empty, P[1], mid, one_key, P[2]]))
            out.append(("p", [P[0], empty, P[1], mid, one_key, P[2], each]))
        out.append(("b", ["b_each_key", B[0], "b_second_empty", "b_second_full", P[0], P[1], B[1]]))
        out.append(("b", [P[1], B[1], B[0], "b_second_empty", "b_second_full", P[0], "b_each_key"]))
        out.append(("b", ["b_second_full", "b_each_key", "b_second_empty", B[0], P[0], B[1], P[1]]))
        out.append(("wp", [P[0], "one_key_wp", P[1], P[2], P[3], empty, one_key]))
        out.append(("wp", [P[2], P[3], empty, all_skip, P[0], P[1], "one_key_wp"]))
    else:
        deep_p, deep_b = "deep_last_slot P", "deep_last_slot B"
        s = {w: "single_%s %s" % (w, g) for w in WS.SINGLES}
        out.append(("p", [deep_p, P[0], empty, P[1], s["tl"], one_key, P[2]]))
        out.append(("p", [P[0], empty, P[1], s["br"], one_key, P[2], deep_p]))
        out.append(("p", [s["tr"], P[3], s["bl"], P[4], s["mid"], all_skip, s["br"]]))
        out.append(("b", [deep_b, B[0], empty, B[1], s["tl"], one_key, P[0]]))
        out.append(("b", [B[0], empty, B[1], s["bl"], one_key, P[0], deep_b]))
        out.append(("b", [deep_b, deep_p, B[0], all_skip, P[1], s["mid"], B[1]]))
    assert all(len(names) == N_BATCH == len(set(names)) for _, names in out)
    return out


def test_submit_equals_the_standard(lib, cases):
    bad, sent = submit_each(lib, list(cases.values()), SLOTS)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert len(sent) == len(cases)


@pytest.mark.parametrize("wgs", WGS_KNOBS)
@pytest.mark.parametrize("band_log2", BAND_KNOBS, ids=lambda v: "band_%s" % (v if v is not None else "unset"))
@pytest.mark.parametrize("geom", [WS.WIDE, WS.DEEP], ids=lambda g: "%dx%d" % g)
def test_batches_equal_the_standard(lib, cases, geom, band_log2, wgs, monkeypatch):
    if band_log2 is None:
        monkeypatch.delenv("P264AMD_MC_BAND_LOG2", raising=False)
    else:
        monkeypatch.setenv("P264AMD_MC_BAND_LOG2", band_log2)
    monkeypatch.setenv("P264AMD_MC_WGS_PER_PIC", wgs)
    plan = orders(geom)
    flat = [cases[name] for _, names in plan for name in names]
    bad, sent, launches = run_batches(lib, flat, n=N_BATCH, road="upload", slots=SLOTS, probe=lambda hip, batch: hip.last_launch())
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert len(launches) == len(plan) and [st.name for st in sent] == [name for _, names in plan for name in names]
    for (what, names), li in zip(plan, launches):
        assert li["pictures"] == N_BATCH, (names, li)
        if wgs == "4":
            assert li["mc_wgs_per_picture"] == 4, (names, li)
        else:
            assert 4 <= li["mc_wgs_per_picture"] <= int(wgs), (names, li)       # (capped by the chunks there can be)
        # which instances ran: a batch of unweighted P pictures carries its edge info in the k_intra_sparse launch; one explicitly
        # weighted picture (k_mc_sort_wp, k_mc_wp) or one B picture (k_mc_sort_b, k_mc_second) sends the whole batch to
        # k_deblock_bs<true>.  The only other way there - a P picture with one frame twice in its list - is ruled out first.
        for name in names:
            d = cases[name][0].pic.desc
            assert len(set(d.ref_slot[:d.n_ref])) == d.n_ref and not int(d.transform_8x8) and not int(d.scaling_lists), name
        kinds = {"wp" if cases[name][0].pic.desc.explicit_wp else "b" if cases[name][0].pic.desc.slice_type == N.SLICE_B else "p" for name in names}
        assert kinds == {"p", what}, (what, names)
        assert (li["edge_info_fused"] > 0) == (what == "p"), (what, names, li)
    assert {what for what, _ in plan} == ({"p", "b", "wp"} if geom == WS.WIDE else {"p", "b"})
