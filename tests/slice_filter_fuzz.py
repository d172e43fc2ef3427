"""Per-macroblock filter offsets at the CPU->GPU seam (TEST INFRASTRUCTURE): pictures of seam_fuzz.make_picture (and
pcm_fuzz.to_ipcm) whose records then get `flags` - the two signed deltas on the picture's alpha_c0_offset / beta_offset
(include/p264hip.h) - and what such a picture decodes to: the oracle's UNFILTERED reconstruction (through pcm_checker, which
composes explicit weights and I_PCM around oracle_reconstruct_nodeblock) followed by tests/slice_filter_checker.py.

A FAMILY is one batch: pictures of one geometry, one stream each, every one a different picture; some carry deltas, some none -
a launch mixes both.  The families are shaped so that each of the three edge-info instances runs (kernel_deblock.h):
plain P batches take the role fused into k_intra_sparse, a batch with an I picture k_deblock_bs<false>, a batch with a B picture, a
list that holds one frame twice or explicit weights k_deblock_bs<true>.

How the deltas are drawn (a picture's `mode`): None - flags stay 0; (per, span) with per "slice" - one pair per slice run, the
runs being the picture's own slices - or "mb" - a pair per macroblock, which the seam permits - and span "int8" - the whole range
-128 .. 127 - or 12 - -12 .. 12, where the indices of most QPs stay inside the tables.
Everything is computed on the CPU; tests/test_slice_filter_cpu.py asserts the coverage, tests/test_gpu_slice_filter_fuzz.py
compares the device with it."""
import numpy as np

from tests import pcm_checker, pcm_fuzz, seam_fuzz
from tests import slice_filter_checker as sfc

SLOTS, DST = 3, 2            # every picture writes slot 2 and reads slots 0, 1

P = dict(n_ref=2, slices=3)
FAMILIES = {
    # name: (mb_w, mb_h, edge-info instance, [(picture kind, make_picture keywords, I_PCM share, mode)])
    "p_plain": (10, 7, "fused", [("p", P, 0, ("slice", 12)), ("p", P, 0, None), ("p", P, 0, ("mb", "int8")), ("p", dict(n_ref=2, slices=4), 0, ("mb", 12)),
                                 ("p", dict(n_ref=1, slices=2, slice_idcs=[0, 2]), 0, ("slice", "int8"))]),
    "p_with_i": (9, 6, "one_list", [("p", P, 0, ("slice", "int8")), ("p", P, 0, None), ("i", dict(slices=3), 0, ("mb", 12)), ("p", P, 0, ("slice", 12)),
                                    ("i", dict(slices=2), 0, ("slice", 12)), ("p", P, 0, ("mb", 12)), ("p", dict(n_ref=1, slices=4), 0, ("mb", 12))]),
    "b_mix": (10, 7, "two_lists", [("b", dict(n_ref=2, n_ref_l1=2, slices=3), 0, ("slice", 12)), ("p", dict(n_ref=3, dup_refs=True, slices=2), 0, ("mb", 12)),
                                   ("b", dict(n_ref=2, n_ref_l1=2, explicit_wp="legal", slices=3), 0, ("slice", "int8")), ("p", P, 0, None),
                                   ("p", dict(n_ref=2, explicit_wp="legal", slices=2), 0, ("mb", 12)), ("b", dict(n_ref=1, n_ref_l1=2, mirror_l1=0.5), 0, ("mb", "int8"))]),
    "p_dup_only": (9, 6, "two_lists", [("p", dict(n_ref=3, dup_refs=True, slices=3), 0, ("slice", 12)), ("p", dict(n_ref=3, dup_refs=True), 0, None),
                                       ("p", P, 0, ("mb", 12))]),
    "pcm_p": (10, 7, "fused", [("p", P, 0.3, ("slice", 12)), ("p", P, 0.3, ("mb", 12)), ("p", dict(n_ref=1), 1.0, ("mb", "int8")), ("p", P, 0.3, None)]),
    "pcm_b_i": (9, 6, "two_lists", [("b", dict(n_ref=2, n_ref_l1=2, slices=3), 0.3, ("slice", 12)), ("i", dict(slices=2), 0.3, ("mb", 12)),
                                    ("p", dict(n_ref=2, explicit_wp="legal", slices=2), 0.3, ("slice", "int8")), ("b", dict(n_ref=1, n_ref_l1=1), 0.3, None)]),
    "single_row": (11, 1, "fused", [("p", dict(n_ref=1, slices=3), 0, ("slice", 12)), ("p", dict(n_ref=1, slices=3), 0, ("mb", 12)), ("p", dict(n_ref=1), 0, None)]),
    "single_column": (1, 9, "one_list", [("p", dict(n_ref=1, slices=4), 0, ("slice", 12)), ("i", dict(slices=3), 0, ("mb", 12)), ("p", dict(n_ref=1, slices=2), 0, None)]),
    # wider than a wavefront: lane 0 of the second wavefront loads its left neighbour instead of taking it from the lane below
    "wide_67": (67, 3, "fused", [("p", P, 0, ("slice", 12)), ("p", P, 0, ("mb", 12)), ("p", P, 0, None)]),
}


def draw_flags(rng, pic, starts, mode):
    """write `flags` into the records of a sealed picture; starts: the first macroblock of every slice"""
    if mode is None:
        return pic
    per, span = mode
    lo, hi = (-128, 128) if span == "int8" else (-int(span), int(span) + 1)
    n = pic.n_mb
    if per == "slice":
        bounds = list(starts) + [n]
        for k in range(len(starts)):
            a, b = (int(x) for x in rng.integers(lo, hi, size=2))
            pic.rec["flags"][bounds[k]:bounds[k + 1]] = sfc.flags_of(a, b)
    else:
        assert per == "mb", per
        ab = rng.integers(lo, hi, size=(n, 2))
        pic.rec["flags"][:] = [sfc.flags_of(int(a), int(b)) for a, b in ab]
    return pic


class Case:
    """one stream of a batch: the picture, its reference frames, the expected planes"""

    def __init__(self, pic, refs, want, mode):
        self.pic, self.refs, self.want, self.mode = pic, refs, want, mode


def expected(oracle, pic, refs, counts=None):
    """the oracle's unfiltered reconstruction, then the checker's filter: [y, u, v] (copies)"""
    chk = pcm_checker.PcmChecker(oracle, pic.mb_w, pic.mb_h, SLOTS)
    for slot, f in enumerate(refs):
        for dst, src in zip(chk.store[slot], f):
            dst[:] = src
    planes = [a.copy() for a in chk.nodeblock(pic)]
    if pic.desc.deblock:
        sfc.deblock(pic, planes, counts)
    return planes


_cache = {}


def family(oracle, name):
    """([Case], Counts) of a family; drawn and computed once per process"""
    if name in _cache:
        return _cache[name]
    mb_w, mb_h, _, specs = FAMILIES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 8713)
    counts = sfc.Counts()
    cases = []
    n = mb_w * mb_h
    for kind, kw, share, mode in specs:
        refs = [seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth") for _ in range(DST)]
        # (the slices' deblocking idcs in turn: every picture filters, slices that keep off their borders and slices that do not filter occur)
        k = dict(level_style="small", qp_mode="random", mv_range=6, intra_share=0.15, slice_idcs=[0, 2, 0, 1])
        k.update(kw)
        slices = k.pop("slices", 1)
        starts = sorted(set([0] + [int(x) for x in rng.integers(1, max(n, 2), size=slices - 1)])) if slices > 1 and n > 1 else [0]
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=kind != "i", b_picture=kind == "b", slots=SLOTS, dst_slot=DST, slice_starts=starts, **k)
        if share:
            pcm_fuzz.to_ipcm(rng, pic, share, samples="frame", src=refs[0], noise=2)
        draw_flags(rng, pic, starts, mode)
        cases.append(Case(pic, refs, expected(oracle, pic, refs, counts), mode))
    _cache[name] = (cases, counts)
    return _cache[name]


def total(oracle, names=None):
    """the Counts of several families added up"""
    out = sfc.Counts()
    for name in names or FAMILIES:
        c = family(oracle, name)[1]
        for a in ("census", "seams", "inner", "tells"):
            getattr(out, a).update(getattr(c, a))
    return out
