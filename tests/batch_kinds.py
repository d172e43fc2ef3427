"""Every kind of picture a batch can hold, and the kernel sets their batches select (TEST INFRASTRUCTURE, no fixtures).

p264hip_reconstruct looks at the whole batch once (batch_fill, p264hip.hip) and plan_launches (csrc/hip/launch_plan.h) picks one
kernel instance per stage for ALL pictures of the call: a picture decodes through different code depending on what shares its call.
This module holds

  KINDS         a table of picture kinds at one geometry (cr_offset_stim.BATCH_W x BATCH_H) and one slot convention (destination 0,
                references 1 and 2), each drawn from a seed through the stimulus helpers that exist and brought into the ranges of
                8.5 under both chroma offsets (cr_offset_checker.make_conformant);
  flags_of      a picture's contribution to BatchKinds, restated from batch_fill;
  plan_rules    the instance of every stage by the batch's kinds, restated from the rules (tests/test_launch_plan_cpu.py pins it
                to the header with a g++ program);
  tuple_of      the instance tuple (sort, mc, second pass, residual, intra, edge-info road, Cr filter) of a set of kinds;
  cover         a deterministic greedy list of subsets of up to four kinds that reaches every reachable (kind, tuple) cell.

Nothing here compiles or starts anything: the GPU test imports it."""
import collections
import functools
import heapq
import itertools

import numpy as np

from p264decoder_amd import _native as N
from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import i8x8_stim as IS
from tests import inter_stim as S
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import seam_fuzz
from tests import stream_args

W, H = CS.BATCH_W, CS.BATCH_H
LARGE_W, LARGE_H = 3, 2           # the geometry of the large batch: every kind still has what its name says (tests/test_batch_kinds_cpu.py)
SLOTS, DST = 3, 0                 # what the High-profile stimulus helpers fix: references in slots 1 and 2, every picture writes slot 0
Stim = collections.namedtuple("Stim", "name pic frames")

# ---- the plan's rules ------------------------------------------------------------------------------------------------------------
FLAGS = ("i", "p", "b", "wp", "dup", "t8", "i8", "sc", "cr")       # BatchKinds; sc and cr: how many pictures (cr: BatchKinds::n_cr)
T8_MBS_PER_WG = 8                 # k_t8x8: 256 threads, one wavefront per two macroblocks
TUPLE = ("sort", "mc", "second", "residual", "intra", "edge", "deblock_cr")


def plan_rules(k, n, bs_knob, n_mb):
    """The plan's enums and the info fields that follow from the kinds alone.  Without p there is no inter stage at all: no sort, no
    motion compensation, no in-place residual (batch_fill sets wp, dup and t8 only for pictures that also set p).  k: {flag: value}
    over FLAGS (cr may be missing: 0); bs_knob: P264AMD_BS_FUSED or None; n_mb: macroblocks per picture."""
    i, p, b, wp, dup, t8, i8, sc = (k[x] for x in FLAGS[:8])
    cr = int(k.get("cr", 0))
    e = {"sort": "none", "mc": "none", "second": 0, "residual": "none"}
    if p:
        if sc:
            e["sort"] = "scaled" if b or wp else "scaled_p"
        elif b:
            e["sort"] = "b_wp" if wp else "b"
        else:
            e["sort"] = "wp" if wp else "plain"
        e["mc"] = "wp" if wp else "plain"
        e["second"] = int(b)
        e["residual"] = "scaled_inter" if sc else "t8x8" if t8 else "none"
    e["t8x8_wgs"] = (n_mb + T8_MBS_PER_WG - 1) // T8_MBS_PER_WG * n if e["residual"] == "t8x8" else 0
    if sc:
        e["intra"] = "dense_scaled" if i else "sparse_scaled"
    elif i8:
        e["intra"] = "dense_i8" if i else "sparse_i8"
    else:
        e["intra"] = "dense" if i else "sparse"
    e["intra_i8"] = int(i8)
    if i or b or wp or dup or t8 or i8 or sc or bs_knob == 0:
        bs_wgs = 0
    else:
        bs_wgs = bs_knob if bs_knob is not None and bs_knob > 0 else 1          # INTRA_BS_WGS = 1
    e["edge_info_fused"] = bs_wgs
    e["edge"] = "bs_true" if b or wp or dup else "fused" if bs_wgs > 0 else "bs_false"
    e["copy_scale_table"] = int(bool(sc))
    e["scaled_pictures"] = sc
    e["pictures"] = n
    # the Cr instances of the loop filter's two launches: any picture with a non-zero cr_qp_offset_delta
    e["deblock_cr"] = int(bool(cr))
    e["cr_pictures"] = cr
    return e


def flags_of(pic):
    """what batch_fill adds to BatchKinds for this picture, from its descriptor"""
    d = pic.desc
    st, t8, delta = int(d.slice_type), int(d.transform_8x8), int(d.cr_qp_offset_delta)
    refs = [int(d.ref_slot[i]) for i in range(min(int(d.n_ref), N.MAX_REFS))]
    return {"i": st == N.SLICE_I, "p": st != N.SLICE_I, "b": st == N.SLICE_B, "wp": bool(int(d.explicit_wp)),
            # (picdev_of: an unweighted P picture whose list 0 holds one frame at two indices)
            "dup": st == N.SLICE_P and not int(d.explicit_wp) and len(set(refs)) < len(refs),
            "t8": bool(t8 & ~N.T8X8_INTRA) and st != N.SLICE_I, "i8": bool(t8 & N.T8X8_INTRA),
            "sc": int(bool(int(d.scaling_lists)) or delta != 0), "cr": int(delta != 0)}


def union(flag_dicts):
    """BatchKinds of a batch: the flags or-ed, sc and cr counted"""
    k = dict.fromkeys(FLAGS, 0)
    for f in flag_dicts:
        for x in FLAGS:
            k[x] = k[x] + int(f[x]) if x in ("sc", "cr") else int(bool(k[x]) or bool(f[x]))
    return k


def tuple_of_flags(flag_dicts, n_mb=W * H):
    flag_dicts = list(flag_dicts)
    e = plan_rules(union(flag_dicts), len(flag_dicts), None, n_mb)
    return tuple(e[x] for x in TUPLE)


# ---- the kinds -------------------------------------------------------------------------------------------------------------------
def _flagged(w, h):
    """the macroblocks that are forced to Intra 8x8: i8x8_stim's cluster at its own geometry, else every fourth macroblock"""
    return IS.CLUSTER if (w, h) == (IS.MB_W, IS.MB_H) else tuple(range(1, w * h, 4))


def _old(kind):
    def make(rng, w, h):
        pic = seam_fuzz.make_picture(rng, w, h, slots=SLOTS, dst_slot=DST, level_style="mixed", qp_mode="random", intra_share=0.2, slices=2,
                                     **stream_args.KINDS[kind])
        return Stim(kind, pic, S.frames_for(rng, w, h, kind="smooth" if rng.random() < 0.5 else "noise"))
    return make


def _p(share=0.0, **kw):
    return lambda rng, w, h: CS.p_picture(rng, w, h, share=share, **kw)


def _b(share=0.0, **kw):
    return lambda rng, w, h: CS.b_picture(rng, w, h, share=share, **kw)


def _i8(t8_share, **kw):
    kw.setdefault("slices", 1)
    kw.setdefault("slice_idcs", [0])
    return lambda rng, w, h: IS.inter_picture(rng, IS.Plan(rng), "", _flagged(w, h), t8_share, mb_w=w, mb_h=h, **kw)


def _i(rng, w, h):
    return CS.i_picture(rng, w, h)


DUP_TELLS = 8                     # samples of a dup-list picture that a loop filter comparing indices would get wrong, at least
Kind = collections.namedtuple("Kind", "name base lists ipcm cqo delta flags has")
# base(rng, w, h) draws the picture; lists: scaling_stim.random_lists seed (Cb and Cr lists that differ) or None; ipcm: a share of the
# macroblocks becomes I_PCM; cqo / delta: chroma_qp_offset (None: as drawn) and cr_qp_offset_delta; flags: per-macroblock deltas on the
# filter offsets; has: what the census (below) must find in the picture
def _k(name, base, has, lists=None, ipcm=False, cqo=None, delta=0, flags=False):
    return Kind(name, base, lists, ipcm, cqo, delta, flags, frozenset(has.split()))


KINDS = [
    # the seven kinds of tests/test_gpu_batch_composition.py (stream_args.KINDS), here with levels inside the ranges of 8.5
    _k("I", _old("I"), "intra"), _k("P", _old("P"), "inter"), _k("P_multi_dup", _old("P_multi_dup"), "inter dup"),
    _k("P_weighted", _old("P_weighted"), "inter wp"), _k("B", _old("B"), "inter"), _k("B_implicit", _old("B_implicit"), "inter"),
    _k("B_weighted", _old("B_weighted"), "inter wp"),
    # the 8x8 transform of inter macroblocks
    _k("P_t8", _p(0.7), "inter t8"), _k("B_t8", _b(0.7), "inter t8"), _k("P_dup_t8", _p(0.7, n_ref=3, dup_refs=True), "inter t8 dup"),
    _k("P_weighted_t8", _p(0.6, explicit_wp="legal"), "inter t8 wp"), _k("B_weighted_t8", _b(0.6, explicit_wp="legal"), "inter t8 wp"),
    # Intra 8x8: among inter macroblocks (without and with T8X8 beside them), and a dense I picture
    _k("P_i8", _i8(0.0), "inter i8"), _k("I_i8", _i, "intra i8"), _k("P_t8_i8", _i8(0.5), "inter t8 i8"),
    _k("B_t8_i8", _i8(0.5, b_picture=True), "inter t8 i8"), _k("B_i8", _i8(0.0, b_picture=True), "inter i8"),
    _k("P_weighted_t8_i8", _i8(0.5, explicit_wp="legal"), "inter t8 i8 wp"),
    # scaling lists whose Cb and Cr lists differ
    _k("P_lists", _p(), "inter lists", lists=41), _k("B_lists", _b(), "inter lists", lists=42), _k("I_lists", _i, "intra i8 lists", lists=43),
    _k("P_weighted_lists", _p(explicit_wp="legal"), "inter wp lists", lists=44), _k("P_dup_lists", _p(n_ref=3, dup_refs=True), "inter dup lists", lists=45),
    _k("P_t8_lists", _p(0.5), "inter t8 lists", lists=52), _k("P_t8_i8_lists", _i8(0.5), "inter t8 i8 lists", lists=46), _k("B_t8_i8_lists", _i8(0.5, b_picture=True), "inter t8 i8 lists", lists=47),
    _k("P_weighted_t8_i8_lists", _i8(0.5, explicit_wp="legal"), "inter t8 i8 wp lists", lists=48),
    # a Cr QP offset of its own, without lists
    _k("P_cr", _p(), "inter cr", cqo=0, delta=-13, flags=True), _k("B_cr", _b(), "inter cr", cqo=12, delta=-24, flags=True),
    _k("I_cr", _i, "intra i8 cr", cqo=-12, delta=24, flags=True),
    _k("P_t8_lists_cr", _p(0.5), "inter t8 lists cr", lists=49, cqo=3, delta=7, flags=True),
    _k("B_t8_cr", _b(0.5), "inter t8 cr", cqo=-5, delta=13, flags=True),
    # I_PCM macroblocks next to coded ones
    _k("P_ipcm", _p(slice_idcs=[0, 0]), "inter ipcm", ipcm=True), _k("B_ipcm", _b(slice_idcs=[0]), "inter ipcm", ipcm=True),
    # everything at once: explicit weights, T8X8, Intra 8x8, lists, I_PCM, per-macroblock filter deltas and a Cr delta
    _k("P_all", _i8(0.5, explicit_wp="legal", n_ref=3, dup_refs=True), "inter wp t8 i8 lists ipcm cr", lists=50, ipcm=True, cqo=-4, delta=9, flags=True),
    _k("B_all", _i8(0.5, b_picture=True, explicit_wp="legal"), "inter wp t8 i8 lists ipcm cr", lists=51, ipcm=True, cqo=6, delta=-11, flags=True),
]
NAMES = [k.name for k in KINDS]
OLD = NAMES[:7]
assert OLD == list(stream_args.KINDS) and len(set(NAMES)) == len(NAMES)
DUP = [k.name for k in KINDS if "dup" in k.has]


def census(pic):
    """what a kind's name promises, counted from the picture's records: a Counter over
    inter / intra: such macroblocks; t8 / i8: inter macroblocks with P264_MB_T8X8 / Intra4x4 records with P264_MB_I8X8 that carry luma
    levels; ipcm: I_PCM macroblocks; dup: the smaller of the quadrant counts at the two indices of list 0 that hold one frame; wp: inter
    macroblocks of a picture with explicit weights; lists: 1 where the lists differ from flat and Cb's from Cr's; cr: the filtered chroma
    edges where QPc(Cr) != QPc(Cb) (cr_offset_checker.reach)"""
    c = collections.Counter()
    d, rec = pic.desc, pic.mb_records()
    inter = rec["mb_type"] > N.MB_IPCM
    coded = (rec["coef_mask"] & 0xffff) != 0
    c["inter"], c["intra"], c["ipcm"] = int(inter.sum()), int((rec["mb_type"] < N.MB_IPCM).sum()), int((rec["mb_type"] == N.MB_IPCM).sum())
    c["t8"] = int((inter & ((rec["intra_modes"] & N.MB_T8X8) != 0) & coded).sum()) if int(d.transform_8x8) & ~N.T8X8_INTRA else 0
    c["i8"] = int(((rec["mb_type"] == N.MB_I4x4) & ((rec["intra_modes"] & N.MB_I8X8) != 0) & coded).sum()) if int(d.transform_8x8) & N.T8X8_INTRA else 0
    c["wp"] = c["inter"] if int(d.explicit_wp) else 0
    refs = [int(d.ref_slot[i]) for i in range(int(d.n_ref))]
    idx = pic.ref_idx.reshape(-1, 4)[inter & (rec["mb_type"] != N.MB_P_SKIP)].reshape(-1)
    for a, b in itertools.combinations(range(len(refs)), 2):
        if refs[a] == refs[b]:
            c["dup"] = max(c["dup"], min(int((idx == a).sum()), int((idx == b).sum())))
    lists = SC.lists_of(pic)
    c["lists"] = int(bool(int(d.scaling_lists)) and lists != [list(x) for x in SC.FLAT] and lists[1] != lists[2] and lists[4] != lists[5])
    if int(d.cr_qp_offset_delta):
        c["cr"] = sum(v for key, v in CR.reach(pic).items() if key[0] == "edge")
    return c


def missing(kind, pic):
    """the names of `kind.has` that the census does not find in the picture, and those it finds although the kind does not name them"""
    c = census(pic)
    extra = {x for x in ("t8", "i8", "dup", "wp", "lists", "cr") if c[x] and x not in kind.has}
    if int(pic.desc.explicit_wp):
        extra.discard("dup")                   # (with explicit weights one frame at two indices is two weights of it, not a flag of the batch)
    return sorted({x for x in kind.has if not c[x]} | {"not " + x for x in extra})


def _near_vectors(rng, pic):
    """a dup-list picture must TELL a comparison by picture from one by index (H.264 8.7.2.1: "different reference pictures"): most
    of its inter macroblocks become four 8x8 partitions whose vectors lie within a quarter sample of one vector of the picture and
    whose quadrants use the two indices of the doubled frame in turn - one picture, vectors closer than four quarter samples: strength
    0 between uncoded blocks, where indices that differ would give 1"""
    d, rec = pic.desc, pic.mb_records()
    refs = [int(d.ref_slot[i]) for i in range(int(d.n_ref))]
    a, b = next((a, b) for a, b in itertools.combinations(range(len(refs)), 2) if refs[a] == refs[b])
    base = rng.integers(-8, 9, size=2)
    mv, ref = pic.mv.reshape(-1, 4, 4, 2), pic.ref_idx.reshape(-1, 4)
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) in (N.MB_P_L0, N.MB_P_8x8) and rng.random() < 0.8:
            rec["mb_type"][m] = N.MB_P_8x8
            for q in range(4):
                mv[m, (q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2] = base + rng.integers(-1, 2, size=2)
            ref[m] = [a, b, b, a] if (m + m // pic.mb_w) & 1 else [b, a, a, b]


def dup_tells(st):
    """whether the picture would come out differently if its loop filter compared list-0 INDICES: the same picture with the doubled
    frame's second index naming a copy of that frame in a slot of its own - what motion compensation reads is the same, the
    reference PICTURES of the two indices differ"""
    d = st.pic.desc
    refs = [int(d.ref_slot[i]) for i in range(int(d.n_ref))]
    b = next(b for a, b in itertools.combinations(range(len(refs)), 2) if refs[a] == refs[b])
    want = expected(st)
    two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, SLOTS + 1)
    for slot, f in st.frames.items():
        two.store.write(slot, f)
    two.store.write(SLOTS, st.frames[refs[b]])
    d.ref_slot[b] = SLOTS
    try:
        other = [p.copy() for p in two.reconstruct(st.pic)]
    finally:
        d.ref_slot[b] = refs[b]
    return int(sum((x != y).sum() for x, y in zip(want, other)))


def v_differs(st):
    """whether Cr's own offset changes a sample of the picture (a 3 x 2 picture can have no chroma level and no filtered edge that tells)"""
    two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, SLOTS)
    for slot, f in st.frames.items():
        two.store.write(slot, f)
    two.reconstruct(st.pic)
    return bool(two.v_differs)


def build(kind, seed, w=W, h=H):
    """the kind's picture from the seed: Stim(name, picture, {slot: frame}).  A draw that lacks what the kind's name says (a 3 x 2
    picture without an I_PCM macroblock, say) is drawn again from the next seed of its own sequence."""
    kind = KINDS[NAMES.index(kind)] if isinstance(kind, str) else kind
    for attempt in range(64):
        rng = np.random.default_rng([seed, NAMES.index(kind.name), attempt])
        st = kind.base(rng, w, h)
        frames = st.frames if st.frames else S.frames_for(rng, w, h)
        if "dup" in kind.has:
            _near_vectors(rng, st.pic)
            frames = S.frames_for(rng, w, h, kind="smooth")                  # (content on which the loop filter works at strength 1)
        st = Stim(kind.name, st.pic, frames)
        rec = st.pic.mb_records()
        if not ((rec["mb_type"] > N.MB_IPCM) & ((rec["intra_modes"] & N.MB_T8X8) != 0)).any():
            st.pic.desc.transform_8x8 = int(st.pic.desc.transform_8x8) & N.T8X8_INTRA      # (t8x8_stim sets it on every picture it draws, share 0 included)
        if kind.lists is not None:
            lists = SS.random_lists(kind.lists)
            assert lists[1] != lists[2] and lists[4] != lists[5]
            SC.set_lists(st.pic, lists)
        if kind.ipcm:
            CS.with_ipcm(rng, st, share=0.2)
        done = CS.finish(st, rng, int(st.pic.desc.chroma_qp_offset) if kind.cqo is None else kind.cqo, kind.delta, name=kind.name, flags=kind.flags)
        if missing(kind, done.pic):
            continue
        if ("cr" not in kind.has or v_differs(Stim(kind.name, done.pic, frames))) and ("dup" not in kind.has or dup_tells(Stim(kind.name, done.pic, frames)) >= DUP_TELLS):
            return Stim(kind.name, done.pic, frames)
    raise AssertionError("%s at %d x %d: no draw has %s" % (kind.name, w, h, sorted(kind.has)))


@functools.lru_cache(maxsize=None)
def pictures(seed=1405, w=W, h=H):
    """{name: Stim} of every kind (drawn once per seed and geometry; the pictures are not to be changed)"""
    return {k.name: build(k, seed, w, h) for k in KINDS}


@functools.lru_cache(maxsize=None)
def kind_flags():
    """{name: flags_of its picture}"""
    return {name: flags_of(st.pic) for name, st in pictures().items()}


def tuple_of(members):
    """the plan's instance tuple (TUPLE) for a batch of one picture of each of the kinds `members` (names)"""
    f = kind_flags()
    return tuple_of_flags([f[m] for m in members])


# ---- the cover -------------------------------------------------------------------------------------------------------------------
def subsets(max_size, names=None):
    names = NAMES if names is None else names
    for size in range(1, max_size + 1):
        yield from itertools.combinations(names, size)


def cells_of(members):
    t = tuple_of(members)
    return {(m, t) for m in members}


def every_tuple():
    """{tuple: a smallest subset that selects it} over subsets of ANY size: the tuple follows from the or of the members' flags, so
    the closure of the kinds' flag sets under union holds them all"""
    f = kind_flags()
    key = lambda fl: tuple(bool(fl[x]) for x in FLAGS)
    seen = {}
    frontier = {}
    for n in NAMES:
        frontier.setdefault(key(f[n]), (n,))
    while frontier:
        seen.update({k: v for k, v in frontier.items() if k not in seen})
        nxt = {}
        for k, members in frontier.items():
            for n in NAMES:
                k2 = tuple(a or b for a, b in zip(k, key(f[n])))
                if k2 not in seen and k2 not in nxt:
                    nxt[k2] = members + (n,)
        frontier = nxt
    out = {}
    for members in sorted(seen.values(), key=lambda m: (len(m), [NAMES.index(x) for x in m])):
        out.setdefault(tuple_of(members), members)
    return out


@functools.lru_cache(maxsize=None)
def cover(max_size=4):
    """subsets of kinds (tuples of names): the singles, the full set, then greedily - most new cells first, ties by order of
    enumeration - subsets of up to max_size until every (kind, tuple) cell that such subsets reach is reached; last, a smallest subset
    for every tuple that only larger subsets select"""
    out = [(n,) for n in NAMES] + [tuple(NAMES)]
    reached = set().union(*(cells_of(m) for m in out))
    # (a heap of (-new cells when last counted, order of enumeration): a count can only fall, so the top entry whose count is still
    # true is the first of those with the most new cells)
    heap = []
    for order, members in enumerate(subsets(max_size)):
        cells = cells_of(members)
        if cells - reached:
            heap.append((-len(cells - reached), order, members, cells))
    heapq.heapify(heap)
    while heap:
        gain, order, members, cells = heapq.heappop(heap)
        new = len(cells - reached)
        if new == -gain:
            out.append(members)
            reached |= cells
        elif new:
            heapq.heappush(heap, (-new, order, members, cells))
    have = {t for _, t in reached}
    out += [members for t, members in every_tuple().items() if t not in have]
    return out


# ---- the expectation -------------------------------------------------------------------------------------------------------------
def expected(st):
    """[y, u, v] of the stimulus from the text of H.264: cr_offset_checker.TwoChains over scaling_checker.SpecRecon, a fresh store
    with the stimulus' frames"""
    two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, SLOTS)
    for slot, f in st.frames.items():
        two.store.write(slot, f)
    want = [p.copy() for p in two.reconstruct(st.pic)]
    assert bool(two.v_differs) == bool(CR.delta_of(st.pic)), "%s: Cr's offset changes nothing" % st.name
    return want
