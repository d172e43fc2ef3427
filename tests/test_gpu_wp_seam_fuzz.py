"""Seam-level fuzz of explicit weighted prediction (H.264 8.4.2.3.2): random weighted P and B pictures built directly at the seam
(tests/seam_fuzz.py, explicit_wp=), decoded by the weighted instances (k_mc_sort_wp, k_mc_sort_b_wp, k_mc_wp, k_deblock_bs<true>)
and checked picture by picture against tests/wp_checker.py - the oracle's motion compensation, the 8.4.2.3.2 formula, then the
oracle's residual and loop filter.  What no stream of the writer carries: sub-4x4 vectors inside B quadrants in both lists, weights
and offsets at the ends of their ranges at every denominator, sums past the 8.4.2.3 limit ("wide"), intra macroblocks beside
weighted ones, slices with every deblocking idc, and reference indices past their list (entry 0 on every road).  Every weighted
picture also goes through the packed and the compact upload, which must give the bytes of p264hip_upload."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import seam_fuzz, wp_checker
from tests.hip_harness import ROADS, compare, reconstructor, through_roads
from tests.wp_seam_stim import CONFIGS, config_inputs

pytestmark = pytest.mark.gpu


def entry(r, n):
    return r if 0 <= r < n else 0


def note(seen, pic, stats):
    """what one picture exercised, into seen"""
    d = pic.desc
    n = pic.n_mb
    is_b = d.slice_type == N.SLICE_B
    inter = pic.rec["mb_type"] > N.MB_IPCM
    mv0 = pic.mv.reshape(n, 4, 4, 2)
    mv1 = pic.mv_l1.reshape(n, 4, 4, 2)
    r0s, r1s = pic.ref_idx.reshape(n, 4), pic.ref_idx_l1.reshape(n, 4)
    seen["past_list"] += int((r0s[inter] >= d.n_ref).sum() + ((r1s[inter] >= d.n_ref_l1).sum() if is_b else 0))
    if not d.explicit_wp:
        return
    tab = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2)
    seen["denoms_y"].add(int(d.wp_log2_denom[0]))
    seen["denoms_c"].add(int(d.wp_log2_denom[1]))
    for k in stats:
        seen[k] += stats[k]
    for m in np.nonzero(inter)[0]:
        for q in range(4):
            qy, qx = (q >> 1) * 2, (q & 1) * 2
            r0, r1 = int(r0s[m, q]), int(r1s[m, q]) if is_b else -1
            u1 = r1 >= 0
            u0 = r0 >= 0 or not u1
            seen["dirs"].add(u0 + 2 * u1)
            used = []
            if u0:
                used.append((0, entry(r0, d.n_ref), mv0[m, qy:qy + 2, qx:qx + 2].reshape(4, 2)))
            if u1:
                used.append((1, entry(r1, d.n_ref_l1), mv1[m, qy:qy + 2, qx:qx + 2].reshape(4, 2)))
            for l, e, v in used:
                seen["phases"] |= {(int(x) & 3, int(y) & 3) for x, y in v.tolist()}
                seen["weights"] |= set(tab[l, e, :, 0].tolist())
                seen["offsets"] |= set(tab[l, e, :, 1].tolist())
            if u0 and u1 and any(len({tuple(x) for x in v.tolist()}) > 1 for _, _, v in used):
                seen["sub8x8_bi"] += 1


def new_seen():
    return dict(past_list=0, denoms_y=set(), denoms_c=set(), dirs=set(), phases=set(), weights=set(), offsets=set(), sub8x8_bi=0,
                clip_low=0, clip_high=0, bi_past_limit=0)


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wp_seam_fuzz(lib, oracle, name, mb_w, mb_h, n_pics, kw):
    slots = kw["slots"]
    chk = wp_checker.WeightedChecker(oracle, mb_w, mb_h, slots)
    with reconstructor(lib, mb_w, mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
        inputs = config_inputs(name, mb_w, mb_h, n_pics, kw)
        for s, f in enumerate(next(inputs)):
            for dst, src in zip(chk.store[s], f):
                dst[:] = src
            hip.write_frame(0, s, *f)
        seen = new_seen()
        for i, pic in enumerate(inputs):
            stats = {}
            want = [a.copy() for a in chk.reconstruct(pic, stats)]
            # (a weighted picture also through the packed and the compact upload: the same bytes)
            through_roads(hip, lib, pic, want, "%s picture %d" % (name, i), ROADS[:3] if pic.desc.explicit_wp else ROADS[:1])
            note(seen, pic, stats)
    big = mb_w * mb_h >= 30
    if kw.get("past_list"):
        assert seen["past_list"] > 20, "hardly any index past its list"
    if not kw.get("explicit_wp"):
        return
    assert seen["denoms_y"] >= {0, 7} and seen["denoms_c"] >= {0, 7}, seen
    assert seen["clip_low"] > 0 and seen["clip_high"] > 0, "the final clip never fired both ways: %s" % seen
    if big:
        assert len(seen["phases"]) == 16, "not every luma quarter-pel phase in weighted blocks: %s" % sorted(seen["phases"])
        assert {-128, 127, 128} <= seen["weights"] and {-128, 127} <= seen["offsets"], "weight / offset ends (or the inferred 2^7) unused"
    if kw.get("b_picture"):
        assert {1, 2, 3} <= seen["dirs"], "not every prediction direction (list 0, list 1, both): %s" % seen["dirs"]
        if big and kw.get("mv_range", 80) < 500:
            assert seen["sub8x8_bi"] > 0, "no bi-predicted quadrant with different vectors inside"
    if kw["explicit_wp"] == "wide":
        assert seen["bi_past_limit"] > 0, "no bi-predicted block whose weight sum breaks the 8.4.2.3 limit"


def test_wp_seam_fuzz_1080p_batch(lib, oracle):
    """one batch of three 1080p streams - weighted P, weighted B, unweighted P - through k_mc_wp at its real scale; the unweighted
    picture decodes through the weighted instances because of its neighbours and must still be the oracle's"""
    rng = np.random.default_rng(20261016)
    mb_w, mb_h, S, slots = 120, 68, 3, 3
    with reconstructor(lib, mb_w, mb_h, n_streams=S, slots=slots, max_pictures=S) as hip:
        chks = [wp_checker.WeightedChecker(oracle, mb_w, mb_h, slots) for _ in range(S)]
        for s in range(S):
            for slot in range(slots):
                f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if slot else "noise")
                for dst, src in zip(chks[s].store[slot], f):
                    dst[:] = src
                hip.write_frame(s, slot, *f)
        kinds = [dict(explicit_wp="legal", intra_share=0.05, wp_denoms=(6, 1)),
                 dict(explicit_wp="legal", intra_share=0.05, b_picture=True, n_ref_l1=2, wp_denoms=(7, 5)),
                 dict(intra_share=0.05)]
        pics = [seam_fuzz.make_picture(rng, mb_w, mb_h, dst_slot=2, n_ref=2, slots=slots, level_style="small", qp_mode="random", **k) for k in kinds]
        hip.upload(0, pics)
        hip.reconstruct(list(range(S)), list(range(S)))
        assert hip.last_launch()["edge_info_fused"] == 0
        for s in range(S):
            compare(hip.read_frame(s, 2), chks[s].reconstruct(pics[s]), "1080p stream %d" % s, pics[s])
