"""The directed pictures of tests/worklist_stim.py prove themselves (CPU): tests/worklist_model.py files every macroblock under its
(band, key) from the documented list rules, and each picture is held to what it is there for - every reachable key of every band
populated and padded as far as the lists' arithmetic allows (below), the highest key of every list in band 31 of 32, one key, no
key, one item, a second pass that is empty or as long as the first.  The conditions are fixed by the rules of the lists, none is measured on a kernel.  The model's
constants, its band rule and the room every list has (mc_layout's max_chunks) come from launch_shared.h / launch_plan.h through the
g++ program of tests/test_launch_plan_cpu.py.  Last, the standard-only model and the CPU oracle agree on every picture: that checks
the stimuli, not the kernels.

Where the arithmetic of the lists rules out "every key holds 1 modulo the chunk" the condition is the nearest one that can hold, with
the reason beside it (worklist_stim's module text): the number of chunks a list needs equals the number of its populated keys - every
key one part-filled chunk - or, for CM under 28 whole macroblocks, the padding is the most its item count can have."""
import collections

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import inter_stim
from tests import residual_checker as RC
from tests import worklist_model as M
from tests import worklist_stim as WS
from tests.test_launch_plan_cpu import CU, K, plan          # noqa: F401 (plan: the fixture that compiles launch_plan.h with g++)
from tests.test_spec_recon_cpu import compare_stims

KNOBS = (0, None, 9)                                        # P264AMD_MC_BAND_LOG2 as tests/test_gpu_worklists.py sets it


@pytest.fixture(scope="module")
def stims():
    out = WS.all_stims()
    for geom in (WS.WIDE, WS.DEEP):
        for b in (False, True):
            st = WS.ordinary(geom, b, 0)
            out[st.name] = st
    return out


def geom_of(st):
    return st.pic.mb_w, st.pic.mb_h


def lists0(st):
    """the lists under band knob 0"""
    return M.lists(st.pic, M.effective_band_log2(st.pic.mb_h, 0))


def bands_of(st):
    return range(M.n_bands(st.pic.mb_h, M.effective_band_log2(st.pic.mb_h, 0)))


def padding(counter, per):
    return M.needed_chunks(counter, per) * per - sum(counter.values())


# ---- the model against the headers ---------------------------------------------------------------------------------------------
def test_model_constants_are_the_headers(plan):
    got = plan([(8, 32, 1, CU, {"p": True}, {})])[0]
    assert (got["MCY_KEYS"], got["MCC_KEYS"], got["MC_MAX_BANDS"], got["ML_LISTS"]) == (M.MCY_KEYS, M.MCC_KEYS, M.MC_MAX_BANDS, len(M.LISTS))
    assert [got["ML_" + l] for l in M.LISTS] == [0, 1, 2, 3]
    for i, l in enumerate(M.LISTS):
        assert (got["chunk_items%d" % i], got["list_keys%d" % i]) == (M.CHUNK[l], M.LIST_KEYS[l]), l
    assert M.MC_KEY_SLOTS == 2 * M.MC_MAX_BANDS * (M.MCY_KEYS + M.MCC_KEYS)
    # the key bits fill the keys of a band exactly; the highest luma key has every bit set
    assert M.PC_GEN | M.MCY_CLAMP | M.MCY_RESID == M.MCY_KEYS - 1 and M.MCC_CLAMP | M.MCC_RESID | M.MCC_BI == M.MCC_KEYS - 1
    assert [M.PC[pc] for pc in ("copy", "h", "v", "diag", "c", "ch", "cv")] == list(range(7))


def test_band_rule_is_launch_device_s(plan):
    cases = [(h, knob) for h in (1, 4, 17, 18, 32, 33, 64, 65, 68, 512) for knob in (None, -1, 0, 1, 4, 9, 10)]
    got = plan([(8, h, 1, CU, {"p": True}, {} if knob is None else {K + "MC_BAND_LOG2": str(knob)}) for h, knob in cases])
    for (h, knob), g in zip(cases, got):
        lg = M.effective_band_log2(h, knob)
        assert (g["band_log2"], g["n_bands"]) == (lg, M.n_bands(h, lg)), (h, knob)
        assert g["n_bands"] <= M.MC_MAX_BANDS
    assert M.effective_band_log2(32, 0) == 0 and M.n_bands(32, 0) == M.MC_MAX_BANDS == 32
    assert M.effective_band_log2(33, 0) == 1                    # the bump: 33 rows are 17 bands of two
    assert M.effective_band_log2(WS.WIDE[1], 0) == 0 and M.n_bands(WS.WIDE[1], 0) == 4


def test_reachable_keys():
    R = M.REACHABLE
    assert len(R["P"][(0, "YM")]) == 28 and len(R["P"][(0, "YQ")]) == 30 and len(R["B"][(0, "YQ")]) == 32
    assert R["B"][(0, "YQ")] == set(range(M.MCY_KEYS)) and R["B"][(1, "YQ")] == R["B"][(1, "YM")] == R["B"][(0, "YM")] == R["P"][(0, "YM")]
    assert all(k & 7 != M.PC_GEN for k in R["P"][(0, "YM")])
    assert R["P"][(0, "YQ")] - R["P"][(0, "YM")] == {M.PC_GEN | M.MCY_CLAMP, M.PC_GEN | M.MCY_CLAMP | M.MCY_RESID}
    assert R["B"][(0, "CQ")] == {0, 1, 2, 3, 4, 6} and R["WP"][(0, "YQ")] == {7, 23} and R["WP"][(0, "CQ")] == {4, 6}
    for kind in R:
        for (ps, l), keys in R[kind].items():
            assert all(0 <= k < M.LIST_KEYS[l] for k in keys)


def test_every_picture_stays_inside_its_reachable_keys(stims):
    for st in stims.values():
        kind = M.kind_of(st.pic)
        for pl, c in lists0(st).items():
            assert M.populated(c) <= M.REACHABLE[kind][pl], (st.name, pl)


# ---- every key of every band ---------------------------------------------------------------------------------------------------
def every_band_reaches(st, L, pl):
    reach = M.REACHABLE[M.kind_of(st.pic)][pl]
    for band in bands_of(st):
        assert M.populated(L[pl], band) == reach, (st.name, pl, band, sorted(reach - M.populated(L[pl], band)))
    return len(reach) * len(bands_of(st))


def test_ym_each_key(stims):
    st = stims["ym_each_key"]
    L = lists0(st)
    assert geom_of(st) == WS.WIDE and len(bands_of(st)) == 4
    n = every_band_reaches(st, L, (0, "YM"))
    assert n == 4 * 28 and set(L[(0, "YM")].values()) == {1}                        # = 1 modulo 4
    assert M.needed_chunks(L[(0, "YM")], 4) == n                                    # one chunk per key: maximum padding
    every_band_reaches(st, L, (0, "CM"))
    assert all(c % 8 == 1 for c in L[(0, "CM")].values())                           # 28 items of a band in four keys, each = 1 modulo 8
    for band in bands_of(st):
        assert sorted(c for (b, k), c in L[(0, "CM")].items() if b == band) == [1, 1, 9, 17]
    assert padding(L[(0, "CM")], 8) == len(L[(0, "CM")]) * 7                        # the most padding 16 keys can have
    assert not L[(0, "YQ")] and not L[(0, "CQ")]
    assert (st.pic.rec["mb_type"] <= N.MB_IPCM).sum() == 4 * 4                      # the rest intra


def test_yq_each_key(stims):
    st = stims["yq_each_key"]
    L = lists0(st)
    n = every_band_reaches(st, L, (0, "YQ"))
    assert n == 4 * 30
    for band in bands_of(st):
        # a P macroblock files four quadrants: 30 keys, 32 items - one key holds 3, every other 1 (= 1 modulo 16)
        assert sorted(c for (b, k), c in L[(0, "YQ")].items() if b == band) == [1] * 29 + [3]
    assert M.needed_chunks(L[(0, "YQ")], 16) == n
    assert every_band_reaches(st, L, (0, "CQ")) == 16
    assert all(c % 4 == 0 and c < 32 for c in L[(0, "CQ")].values())               # (four entries per macroblock: never 1 modulo 32)
    assert M.needed_chunks(L[(0, "CQ")], 32) == 16
    assert not L[(0, "YM")] and not L[(0, "CM")]


def test_b_each_key(stims):
    st = stims["b_each_key"]
    L = lists0(st)
    assert st.pic.desc.slice_type == N.SLICE_B and st.pic.desc.weighted_bipred == 1
    assert every_band_reaches(st, L, (0, "YQ")) == 4 * 32 and every_band_reaches(st, L, (1, "YQ")) == 4 * 28
    assert every_band_reaches(st, L, (0, "CQ")) == 4 * 6 and every_band_reaches(st, L, (1, "CQ")) == 4 * 4
    assert set(L[(1, "YQ")].values()) == {1}                                        # second pass: = 1 modulo 16
    assert all(c < 16 for c in L[(0, "YQ")].values())                               # first pass: one part-filled chunk per key
    assert M.needed_chunks(L[(0, "YQ")], 16) == 4 * 32 and M.needed_chunks(L[(1, "YQ")], 16) == 4 * 28
    # the chroma quadrant lists of both passes - the second carries the MCE_KEEP entries: one part-filled chunk per key too
    for ps in (0, 1):
        assert all(c % 4 == 0 and c < 32 for c in L[(ps, "CQ")].values()), ps
        assert M.needed_chunks(L[(ps, "CQ")], 32) == len(L[(ps, "CQ")]) == 4 * (6, 4)[ps], ps
    assert not any(L[(ps, l)] for ps in (0, 1) for l in ("YM", "CM"))
    # carried chroma entries beside real ones: 14 macroblocks per band with two quadrants that are not the second pass's
    assert M.keep_entries(st.pic) == 4 * 14 * 2
    roads = collections.Counter(inter_stim.IC.classify(st.pic, int(m))[1] for m in np.flatnonzero(st.pic.rec["mb_type"] > N.MB_IPCM))
    assert roads == {"second pass with carried quadrants": 4 * 14, "list0 only": 4, "generic": 8}
    r0, r1 = st.pic.ref_idx.reshape(-1, 4), st.pic.ref_idx_l1.reshape(-1, 4)
    assert ((r0 >= 0) & (r1 < 0)).any() and ((r0 < 0) & (r1 >= 0)).any() and ((r0 >= 0) & (r1 >= 0)).any()


# ---- 32 bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["P", "B"])
def test_deep_last_slot(stims, kind):
    st = stims["deep_last_slot " + kind]
    L = lists0(st)
    assert geom_of(st) == WS.DEEP and M.effective_band_log2(WS.DEEP[1], 0) == 0 and len(bands_of(st)) == M.MC_MAX_BANDS == 32
    assert len(L) == (8 if kind == "B" else 4)
    for pl, c in L.items():
        reach = M.REACHABLE[kind][pl]
        assert max(reach) in M.populated(c, 31), (pl, "highest key in the last band")
        assert M.populated(c, 0), (pl, "band 0")
        assert M.populated(c) == reach, (pl, sorted(reach - M.populated(c)))
    # the last key slot of the sort that any picture reaches: chroma quadrants, band 31, MCC_BI | MCC_RESID
    if kind == "B":
        assert (31, M.MCC_BI | M.MCC_RESID) in L[(0, "CQ")] and (31, M.MCY_KEYS - 1) in L[(0, "YQ")]


# ---- one key, no key, one item, the second pass ----------------------------------------------------------------------------------
def keys_per_band(st, pl):
    L = lists0(st)
    return [len(M.populated(L[pl], band)) for band in bands_of(st)]


@pytest.mark.parametrize("geom", [WS.WIDE, WS.DEEP])
def test_one_key_and_empty(stims, geom):
    st = stims["one_key %dx%d" % geom]
    L = lists0(st)
    assert set(keys_per_band(st, (0, "YM"))) == {1} and set(keys_per_band(st, (0, "CM"))) == {1}
    assert M.populated(L[(0, "YM")]) == {0} and M.populated(L[(0, "CM")]) == {0} and not L[(0, "YQ")] and not L[(0, "CQ")]
    assert sum(L[(0, "YM")].values()) == geom[0] * geom[1] and not st.pic.desc.n_coef_blocks
    assert set(st.pic.rec["mb_type"].tolist()) == {N.MB_P_SKIP} and not st.pic.ref_idx.any()
    # vector 0 everywhere: the windows of the border macroblocks reach over it - the one key and its clamped twin
    st = stims["all_skip %dx%d" % geom]
    L = lists0(st)
    assert not st.pic.mv.any() and M.populated(L[(0, "YM")]) == {0, M.MCY_CLAMP} and M.populated(L[(0, "CM")]) == {0, M.MCC_CLAMP}
    inner = (geom[0] - 2) * (geom[1] - 2)
    assert sum(c for (b, k), c in L[(0, "YM")].items() if k == 0) == inner
    st = stims["empty %dx%d" % geom]
    assert st.pic.desc.slice_type == N.SLICE_P and (st.pic.rec["mb_type"] <= N.MB_IPCM).all()
    assert all(not c for c in lists0(st).values())


def test_one_key_wp(stims):
    st = stims["one_key_wp"]
    L = lists0(st)
    assert st.pic.desc.explicit_wp and (st.pic.rec["mb_type"] > N.MB_IPCM).all() and geom_of(st) == WS.WIDE
    assert M.populated(L[(0, "YQ")]) == {M.PC_GEN, M.PC_GEN | M.MCY_RESID} and len(M.populated(L[(0, "YQ")])) == 2
    assert M.populated(L[(0, "CQ")]) == {M.MCC_BI, M.MCC_BI | M.MCC_RESID}
    assert not L[(0, "YM")] and not L[(0, "CM")] and sum(L[(0, "YQ")].values()) == sum(L[(0, "CQ")].values()) == 4 * 128


def test_singles(stims):
    w, h = WS.DEEP
    at = {"tl": 0, "tr": w - 1, "bl": (h - 1) * w, "br": w * h - 1}
    for where, m in at.items():
        st = stims["single_%s %dx%d" % (where, w, h)]
        L = lists0(st)
        assert np.flatnonzero(st.pic.rec["mb_type"] > N.MB_IPCM).tolist() == [m] and st.pic.rec["coef_mask"][m] & 0xffff
        # one item: 3 padding entries behind it in YM, 7 in CM
        assert dict(L[(0, "YM")]) == {(m // w, 30): 1} and dict(L[(0, "CM")]) == {(m // w, 3): 1} and not L[(0, "YQ")] and not L[(0, "CQ")]
        assert padding(L[(0, "YM")], 4) == 3 and padding(L[(0, "CM")], 8) == 7
    for geom in (WS.WIDE, WS.DEEP):
        st = stims["single_mid %dx%d" % geom]
        L = lists0(st)
        inter = np.flatnonzero(st.pic.rec["mb_type"] > N.MB_IPCM).tolist()
        assert inter == [(geom[1] // 2) * geom[0] + geom[0] // 2]
        # one macroblock's four quadrants under one key: 12 padding entries in YQ, 28 in CQ
        assert list(L[(0, "YQ")].values()) == [4] and list(L[(0, "CQ")].values()) == [4] and not L[(0, "YM")] and not L[(0, "CM")]
        assert padding(L[(0, "YQ")], 16) == 12 and padding(L[(0, "CQ")], 32) == 28


def test_second_pass_empty_and_full(stims):
    st = stims["b_second_empty"]
    L = lists0(st)
    assert st.pic.desc.slice_type == N.SLICE_B and len(L) == 8
    assert all(not L[(1, l)] for l in M.LISTS) and all(L[(0, l)] for l in M.LISTS)
    assert (st.pic.ref_idx_l1 >= 0).any() and not ((st.pic.ref_idx >= 0) & (st.pic.ref_idx_l1 >= 0)).any()
    st = stims["b_second_full"]
    L = lists0(st)
    assert ((st.pic.ref_idx >= 0) & (st.pic.ref_idx_l1 >= 0)).all()
    for l in M.LISTS:
        assert L[(0, l)] and sum(L[(1, l)].values()) == sum(L[(0, l)].values()), l
        assert len(L[(1, l)]) == len(L[(0, l)]), l
        assert [len(M.populated(L[(1, l)], b)) for b in bands_of(st)] == [len(M.populated(L[(0, l)], b)) for b in bands_of(st)]
    assert M.keep_entries(st.pic) == 0


# ---- every picture --------------------------------------------------------------------------------------------------------------
def test_every_list_fits_its_room(plan, stims):
    """needed_chunks <= mc_layout's max_chunks for every picture, pass and list, under each band knob the GPU test sets"""
    cases = [(geom, knob) for geom in (WS.WIDE, WS.DEEP) for knob in KNOBS]
    got = plan([(w, h, 1, CU, {"p": True}, {} if knob is None else {K + "MC_BAND_LOG2": str(knob)}) for (w, h), knob in cases])
    room = dict(zip(cases, got))
    tight = {}
    for st in stims.values():
        for knob in KNOBS:
            g = room[(geom_of(st), knob)]
            lg = M.effective_band_log2(st.pic.mb_h, knob)
            assert g["band_log2"] == lg
            for (ps, l), c in M.lists(st.pic, lg).items():
                need, have = M.needed_chunks(c, M.CHUNK[l]), g["max_chunks%d" % (ps * len(M.LISTS) + M.LISTS.index(l))]
                assert need <= have, (st.name, knob, ps, l, need, have)
                tight[(ps, l)] = max(tight.get((ps, l), 0), need)
    # the bound is the padding bound: every key one part-filled chunk more than the items fill (launch_shared.h, mc_layout)
    for (w, h), knob in cases:
        g, nb = room[((w, h), knob)], M.n_bands(h, M.effective_band_log2(h, knob))
        for ps in (0, 1):
            for i, l in enumerate(M.LISTS):
                items = w * h * (1 if l in ("YM", "CM") else 4)
                assert g["max_chunks%d" % (ps * 4 + i)] == (items + nb * M.LIST_KEYS[l] * (M.CHUNK[l] - 1)) // M.CHUNK[l] + 1
    assert all(tight[pl] > 0 for pl in tight)


def test_the_gpu_batches_hold_every_directed_picture():
    """tests/test_gpu_worklists.py: every directed picture rides in a batch of its geometry, with a successor behind it and as the
    last picture of a batch wherever it is one of the extreme ones"""
    from tests.test_gpu_worklists import N_BATCH, orders
    directed = WS.all_stims()
    seen, last, followed = set(), set(), set()
    for geom in (WS.WIDE, WS.DEEP):
        for what, names in orders(geom):
            assert len(names) == N_BATCH
            for name in names:
                assert name.startswith("ordinary") or geom_of(directed[name]) == geom, name
            seen |= set(names)
            last.add(names[-1])
            followed |= {a for a, b in zip(names, names[1:]) if b.startswith("ordinary")}
    assert seen >= set(directed)
    extreme = {"ym_each_key", "yq_each_key", "b_each_key", "one_key_wp", "deep_last_slot P", "deep_last_slot B"}
    assert extreme <= last and extreme <= followed


def test_pictures_are_conformant_and_within_the_vector_limits(stims):
    for st in stims.values():
        assert not RC.census(st.pic)[1], st.name
        rec = st.pic.mb_records()
        for m in np.flatnonzero(rec["coef_mask"]):
            mask = int(rec["coef_mask"][m])
            for bit in range(26):
                if mask >> bit & 1:
                    assert np.any(RC.levels_of(st.pic, rec[m], 1 << bit)), (st.name, int(m), bit, "a coded block without a level")
        for mv in (st.pic.mv.reshape(-1, 2), st.pic.mv_l1.reshape(-1, 2)):
            assert mv[:, 0].min() >= inter_stim.LIMITS_X[0] and mv[:, 0].max() <= inter_stim.LIMITS_X[-1], st.name
            assert mv[:, 1].min() >= inter_stim.LIMITS_Y[0] and mv[:, 1].max() <= inter_stim.LIMITS_Y[-1], st.name


def test_standard_and_oracle_agree_on_every_picture(oracle, stims):
    assert WS.SLOTS == 3
    bad = compare_stims(oracle, list(stims.values()))
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])
