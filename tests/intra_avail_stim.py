"""The drawn batches behind tests/test_gpu_intra_avail.py and its CPU twins: pictures of seam_fuzz.make_picture(avail_mode="free")
and seam_fuzz.make_directed per family, what tests/intra_checker.py makes of them, and the coverage they must reach."""
import numpy as np

from p264decoder_amd import _native as N
from tests import intra_checker, pcm_fuzz, seam_fuzz

SLOTS, DST, S = 3, 2, 3
ROADS = ("upload", "packed", "compact")
FAMILIES = {
    # name: (mb_w, mb_h, I_PCM share, make_picture keywords); "directed": seam_fuzz.make_directed instead of the free flags
    "p": (20, 12, 0.0, dict(n_ref=2)),
    "b": (20, 12, 0.0, dict(n_ref=2, n_ref_l1=2, b_picture=True)),
    "b_weighted": (10, 8, 0.0, dict(n_ref=2, n_ref_l1=2, b_picture=True, explicit_wp="legal")),
    "p_ipcm": (20, 12, 0.3, dict(n_ref=2)),
    "b_ipcm": (20, 12, 0.3, dict(n_ref=2, n_ref_l1=2, b_picture=True)),
    "p_sliced_ipcm": (16, 10, 0.2, dict(n_ref=1, slices=3)),
    # a quarter of the macroblocks intra: most of them wait for exactly one round (road 1 of k_intra_sparse)
    "p_quarter": (30, 17, 0.15, dict(n_ref=1, shares=(0.2, 0.25, 0.3))),
    "p_quarter_no_ipcm": (30, 17, 0.0, dict(n_ref=2, shares=(0.2, 0.25, 0.3))),
    "b_quarter": (30, 17, 0.15, dict(n_ref=1, n_ref_l1=1, b_picture=True, shares=(0.2, 0.25, 0.3))),
    "p_single_row": (11, 1, 0.2, dict(n_ref=1)),
    "p_single_column": (1, 9, 0.2, dict(n_ref=1)),
    "p_wide_67": (67, 3, 0.2, dict(n_ref=2)),
    "p_directed": (9, 7, 0.0, dict(n_ref=2, directed=True)),
    "b_directed": (9, 7, 0.0, dict(n_ref=2, n_ref_l1=2, b_picture=True, directed=True)),
}
INTRA_SHARES = (0.1, 0.25, 0.6)           # per stream of a batch: few intra macroblocks -> ready at once, many -> the ordered band walk


def draw(name, with_i):
    """the pictures of a family's batch: [(picture, reference frame, forced macroblock or None)] per stream"""
    mb_w, mb_h, share, kw = FAMILIES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 977 + with_i)
    kw = dict(kw)
    directed, shares = kw.pop("directed", False), kw.pop("shares", INTRA_SHARES)
    out = []
    for s in range(S):
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "noise")
        is_i = with_i and s == S - 1
        k = dict(kw)
        if is_i:
            k = {a: b for a, b in k.items() if a not in ("b_picture", "n_ref_l1", "explicit_wp")}
        k.update(p_picture=not is_i, slots=SLOTS, dst_slot=DST, intra_share=shares[s], level_style="mixed", qp_mode="random")
        if directed:
            pic, target = seam_fuzz.make_directed(rng, mb_w, mb_h, ("i16", "i4", "i16")[(s + with_i) % 3], **k)
        else:
            pic, target = seam_fuzz.make_picture(rng, mb_w, mb_h, avail_mode="free", **k), None
            if share:
                pcm_fuzz.to_ipcm(rng, pic, share)
        out.append((pic, f, target))
    return out


def prepare(oracle, name, with_i):
    """... and what the intra checker makes of them: [(picture, reference frame, expected planes)], the checker's DC log of the
    directed macroblocks [(macroblock, which, mb_type, DC, DC of the left column alone)]"""
    mb_w, mb_h = FAMILIES[name][:2]
    batch, log = [], []
    for pic, f, target in draw(name, with_i):
        chk = intra_checker.IntraChecker(oracle, mb_w, mb_h, SLOTS)
        for slot in range(DST):
            for dst, src in zip(chk.store[slot], f):
                dst[:] = src
        batch.append((pic, f, [a.copy() for a in chk.reconstruct(pic)]))
        log += [e for e in chk.dc_log if e[0] == target]
    return batch, log


def survey_all():
    """the coverage of every family's two batches and of the 1080p batch, from the drawn pictures alone"""
    seen = intra_checker.new_survey()
    for name in FAMILIES:
        for with_i in (False, True):
            for pic, f, target in draw(name, with_i):
                intra_checker.survey(pic, seen, dense=bool(with_i))
    for pic, f, target in draw_1080p():
        intra_checker.survey(pic, seen, dense=False)
    return seen


def check_coverage(seen):
    """every assertion of the coverage list, nothing excluded"""
    both = {(False, False), (False, True), (True, False), (True, True)}
    for t, what in ((N.MB_I16x16, "Intra16x16"), (N.MB_I4x4, "Intra4x4"), (N.MB_IPCM, "I_PCM")):
        for road in (0, 1, 2, "dense"):
            got = {a for tt, r, a in seen["avail"] if tt == t and r == road}
            assert got == set(range(16)), "%s, %s: flag combinations %s never drawn" % (what, "road %s" % road, sorted(set(range(16)) - got))
    assert seen["i16_dc"] == both, seen["i16_dc"]
    assert seen["chroma_dc"] == both, seen["chroma_dc"]
    assert seen["i4_block0_dc"] == both, seen["i4_block0_dc"]
    assert seen["i4_tr_missing_mb"] == {3, 7}, seen["i4_tr_missing_mb"]
    assert seen["i4_tr_missing_inside"] == {3, 7}, seen["i4_tr_missing_inside"]


def check_directed(name, with_i, batch, log):
    """every picture of a directed family has its macroblock with LEFT, TOP and no TOPLEFT, Intra16x16 DC or Intra4x4, chroma DC,
    and there the DC of the standard differs from the DC of the left column alone (what the parent's kernels predicted)"""
    kinds = set()
    for pic, f, want in batch:
        rec = pic.rec
        m = [int(x) for x in np.flatnonzero(((rec["avail"] & 11) == 3) & (rec["mb_type"] <= N.MB_I16x16) & ((rec["intra_modes"] >> 4) == 0))]
        mine = [e for e in log if e[0] in m]
        assert m and mine, "%s: no such macroblock" % name
        kinds |= {(e[1], e[2]) for e in mine}
        assert all(abs(e[3] - e[4]) > 20 for e in mine), mine
    assert kinds >= {("i16", N.MB_I16x16), ("cb", N.MB_I16x16), ("cr", N.MB_I16x16), ("cb", N.MB_I4x4), ("cr", N.MB_I4x4)}, kinds


def draw_1080p():
    """one batch of 1080p pictures: P, B and P with I_PCM; small intra shares (the Python checker walks every intra macroblock)"""
    rng = np.random.default_rng(10801)
    mb_w, mb_h = 120, 68
    out = []
    for kw, share, pcm in [(dict(n_ref=2), 0.03, 0.0), (dict(n_ref=2, n_ref_l1=2, b_picture=True), 0.06, 0.0), (dict(n_ref=1), 0.05, 0.03)]:
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "noise")
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, slots=SLOTS, dst_slot=DST, intra_share=share, level_style="small", avail_mode="free", **kw)
        if pcm:
            pcm_fuzz.to_ipcm(rng, pic, pcm)
        out.append((pic, f, None))
    return out
