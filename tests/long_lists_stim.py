"""Pictures whose reference lists hold up to 16 entries, in a frame store of 17 slots (TEST INFRASTRUCTURE), built at the CPU->GPU
seam from seeds.  include/p264hip.h admits 16 entries per list and P264HIP_MAX_REFS + 1 slots per stream; the index travels as a
4-bit field through the work lists of kernel_mc_sort.h, the 2 x 16 tables of kernel_mc.h and kernel_deblock.h and the 16 x 16
implicit weights, and none of the other stimulus modules goes past 4.

`pictures()`: 8 x 6 macroblocks, every slot of the store with content of its own (seam_fuzz.random_frame), the destination slot 0
or 16 in turn:

  P <n>               n = 16, 15, 9, 8, 5 distinct entries (the steps round bit 3 of the index and the last index);
  P wp 16             explicit weights, every (entry, plane) with a pair of its own (seam_fuzz.draw_wp_table);
  P dup 16            entries 11 and 14 name the slot of entry 2; most macroblocks are four 8x8 partitions with vectors within a
                      quarter sample of each other that use the three indices in turn: one picture through different indices, strength
                      0 by H.264 8.7.2.1 where a comparison of indices gives 1;
  B / B implicit /    16 + 16 entries, list 1 the slots of list 0 the other way round; `crossed` neighbours reach one pair of
  B wp                pictures through different (list, index) with the vectors swapped (strength 0 by picture, 1 by index);
  B 16+1, 1+16, 9+7   lists of unequal length;
  P lists / B lists   scaling lists (scaling_checker): the batch's sort is k_mc_sort_scaled_p / k_mc_sort_scaled;
  P cr                a cr_qp_offset_delta (cr_offset_checker): k_deblock_bs_cr;
  P t8 / B t8         P264_MB_T8X8 records (t8x8_checker).

What make_picture draws leaves entries of a 16-entry list without a whole-macroblock item (a B macroblock draws list 1's entry per
quadrant), so `spread` walks the macroblocks that are one item per list and deals them the entries of each list in turn, and
`pin_pairs` gives bi-predicted quadrants the pairs PINNED: (15, 15) and every index from 8 of both lists.  `assert_covered` states what the SET
reaches; `WRONG` holds the deliberately wrong copies of the REFERENCE that show each stimulus can notice the faults the set
is about (tests/test_long_lists_cpu.py)."""
import collections
import ctypes as C
import functools

import numpy as np

from p264decoder_amd import _native as N
from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import deblock_checker as DC
from tests import inter_checker as IC
from tests import residual_checker as RC
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import seam_fuzz
from tests import spec_recon
from tests import t8x8_checker as T8

W, H, SLOTS = 8, 6, 17
SEED = 1617
DUP = (2, 11, 14)                 # the indices of "P dup 16" that name one slot
PINNED = ((15, 15), (15, 8), (8, 15)) + tuple((8 + k, 8 + (3 * k + 1) % 8) for k in range(8))     # every high index of both lists
Stim = collections.namedtuple("Stim", "name pic frames kept checker")     # checker: "spec" | "scaling" | "cr" | "t8x8"


# ---- drawing -----------------------------------------------------------------------------------------------------------------------
def frames_for(rng, kind="noise"):
    """{slot: [y, u, v]} for every slot of the store, each drawn on its own"""
    return {s: seam_fuzz.random_frame(rng, W, H, kind) for s in range(SLOTS)}


def _one_item_lists(pic, m):
    """the lists macroblock m uses if it is ONE item per list - every quadrant the same lists, one vector per list - else None"""
    d = pic.desc
    is_b = d.slice_type == N.SLICE_B
    r0, r1 = pic.ref_idx.reshape(-1, 4)[m], pic.ref_idx_l1.reshape(-1, 4)[m]
    use0 = [int(x) >= 0 for x in r0]
    use1 = [is_b and int(x) >= 0 for x in r1]
    if len(set(use0)) != 1 or len(set(use1)) != 1 or not (use0[0] or use1[0]):
        return None
    for use, mv in ((use0[0], pic.mv), (use1[0], pic.mv_l1)):
        if use and len({tuple(v) for v in mv.reshape(-1, 16, 2)[m].tolist()}) != 1:
            return None
    return use0[0], use1[0]


def spread(pic, cursor):
    """the macroblocks that are one item per list get the entries of each list dealt in turn - list 0 upwards, list 1 downwards, from
    where `cursor` ([next of list 0, next of list 1], carried through the set) stands, so the pairs vary and the dealing goes on
    where the picture before stopped: every entry of a 16-entry list meets a whole-macroblock item"""
    d, rec = pic.desc, pic.mb_records()
    ref = [pic.ref_idx.reshape(-1, 4), pic.ref_idx_l1.reshape(-1, 4)]
    n = [int(d.n_ref), int(d.n_ref_l1) if d.slice_type == N.SLICE_B else 0]
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) not in (N.MB_P_L0, N.MB_B):
            continue
        lists = _one_item_lists(pic, m)
        if lists is None:
            continue
        for l in (0, 1):
            if lists[l]:
                ref[l][m] = cursor[l] % n[l]
                cursor[l] += (1, -1)[l]


def pin_pairs(pic):
    """bi-predicted quadrants of macroblocks that go through the second pass quadrant by quadrant get the pairs PINNED, in turn"""
    todo = list(PINNED)
    r0, r1 = pic.ref_idx.reshape(-1, 4), pic.ref_idx_l1.reshape(-1, 4)
    for m in range(pic.n_mb):
        if int(pic.mb_records()["mb_type"][m]) != N.MB_B or IC.classify(pic, m)[1] not in ("second pass quadrants", "second pass with carried quadrants"):
            continue
        for q in range(4):
            if todo and r0[m, q] >= 0 and r1[m, q] >= 0:
                r0[m, q], r1[m, q] = todo.pop(0)
    assert not todo, "no bi-predicted quadrants left for %s" % (todo,)


def skew_weights(rng, pic):
    """bipred_weight[a][b] != bipred_weight[b][a] for every a != b: a table read the wrong way round is a different table"""
    d = pic.desc
    for a in range(N.MAX_REFS):
        for b in range(a + 1, N.MAX_REFS):
            while int(d.bipred_weight[a * N.MAX_REFS + b]) == int(d.bipred_weight[b * N.MAX_REFS + a]):
                d.bipred_weight[b * N.MAX_REFS + a] = int(rng.integers(-64, 129))


def near_vectors(rng, pic, indices=DUP):
    """most inter macroblocks become four 8x8 partitions whose vectors lie within a quarter sample of one vector of the picture and
    whose quadrants use `indices` (one slot) in turn"""
    rec = pic.mb_records()
    base = rng.integers(-8, 9, size=2)
    mv, ref = pic.mv.reshape(-1, 4, 4, 2), pic.ref_idx.reshape(-1, 4)
    k = 0
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) in (N.MB_P_L0, N.MB_P_8x8) and rng.random() < 0.8:
            rec["mb_type"][m] = N.MB_P_8x8
            for q in range(4):
                mv[m, (q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2] = base + rng.integers(-1, 2, size=2)
                ref[m, q] = indices[(k + q + (q >> 1)) % len(indices)]
            k += 1


def crossed(rng, pic):
    """macroblocks without luma levels become four bi-predicted quadrants that reach the same two pictures through different
    (list, index), vectors swapped with the pictures, in a checkerboard: list 0 entry i with va and list 1 entry j with vb beside
    list 0 entry n - 1 - j (list 1's picture) with vb + 1 and list 1 entry n - 1 - i (list 0's picture) with va - 1.  List 1 holds
    list 0's slots the other way round (make_picture): entry i of list 0 is entry n - 1 - i of list 1.  Returns the macroblocks."""
    d, rec = pic.desc, pic.mb_records()
    n = int(d.n_ref)
    assert n == int(d.n_ref_l1) and all(int(d.ref_slot[i]) == int(d.ref_slot_l1[n - 1 - i]) for i in range(n))
    mv = [pic.mv.reshape(-1, 4, 4, 2), pic.mv_l1.reshape(-1, 4, 4, 2)]
    ref = [pic.ref_idx.reshape(-1, 4), pic.ref_idx_l1.reshape(-1, 4)]
    done = 0
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) != N.MB_B or int(rec["coef_mask"][m]) & 0xffff or rng.random() >= 0.8:
            continue
        i, j = 8 + done % 8, int(rng.integers(0, n))
        while n - 1 - j == i:
            j = int(rng.integers(0, n))
        va, vb = rng.integers(-12, 13, size=2), rng.integers(-12, 13, size=2)
        for q in range(4):
            ys, xs = slice((q >> 1) * 2, (q >> 1) * 2 + 2), slice((q & 1) * 2, (q & 1) * 2 + 2)
            if q in (0, 3):
                ref[0][m, q], ref[1][m, q], mv[0][m, ys, xs], mv[1][m, ys, xs] = i, j, va, vb
            else:
                ref[0][m, q], ref[1][m, q], mv[0][m, ys, xs], mv[1][m, ys, xs] = n - 1 - j, n - 1 - i, vb + 1, va - 1
        done += 1
    return done


def mild_wp(rng, pic):
    """explicit weights near the default ones - denominator 5, weights 28 .. 36, offsets -6 .. 6, every (list, entry, plane) a pair of
    its own: two predictions of one picture stay close enough for the loop filter to work between them"""
    d = pic.desc
    t = np.zeros((2, N.MAX_REFS, 3, 2), np.int64)
    seen = set()
    for idx in np.ndindex(2, N.MAX_REFS, 3):
        while True:
            pair = (int(rng.integers(28, 37)), int(rng.integers(-6, 7)))
            if (idx[2], pair) not in seen:
                break
        seen.add((idx[2], pair))
        t[idx] = pair
    d.explicit_wp, d.weighted_bipred = 1, 0
    d.wp_log2_denom[0], d.wp_log2_denom[1] = 5, 5
    np.ctypeslib.as_array(d.wp)[:] = t.reshape(-1).astype(np.int16)


def _plain(name, seed, dst, cursor, frames="noise", dup=False, cross=False, wp=None, **kw):
    rng = np.random.default_rng([SEED, seed])
    b = bool(kw.get("b_picture"))
    kw.setdefault("mirror_l1", 0.25 if b else 0.0)
    kw.setdefault("qp_mode", "random")
    pic = seam_fuzz.make_picture(rng, W, H, slots=SLOTS, dst_slot=dst, level_style="small", intra_share=0.1, slices=2, slice_idcs=[0, 2], **kw)
    if cross:
        assert crossed(rng, pic) >= 8, name
    if dup:
        for i in DUP[1:]:
            pic.desc.ref_slot[i] = pic.desc.ref_slot[DUP[0]]
        near_vectors(rng, pic)
    spread(pic, cursor)                              # (the macroblocks `crossed` and `near_vectors` made are not one item)
    if b and int(pic.desc.n_ref) == 16 and int(pic.desc.n_ref_l1) == 16:
        pin_pairs(pic)
    if b:
        skew_weights(rng, pic)
    if wp == "mild":
        mild_wp(rng, pic)
    elif wp:
        seam_fuzz.draw_wp_table(rng, pic, wp)
    kept = RC.make_conformant(pic) if pic.desc.n_coef_blocks else (0, 0)
    return Stim(name, pic, frames_for(rng, frames), kept, "spec")


def _high(name, seed, dst, checker, b=False, share=0.0, lists=None, cqo=None, delta=0):
    """a picture by the High-profile stimulus helpers (tests/cr_offset_stim.py) with 16-entry lists"""
    rng = np.random.default_rng([SEED, seed])
    draw = CS.b_picture if b else CS.p_picture
    st = draw(rng, W, H, share=share, n_ref=16, n_ref_l1=16, slots=SLOTS, dst_slot=dst, **({"mirror_l1": 0.25} if b else {}))
    pic = st.pic
    if b:
        skew_weights(rng, pic)
    if not share:
        pic.desc.transform_8x8 = 0                   # (t8x8_stim sets it on every picture it draws, share 0 included)
    if lists is not None:
        SC.set_lists(pic, SS.random_lists(lists))
    pic.desc.chroma_qp_offset = int(pic.desc.chroma_qp_offset) if cqo is None else cqo
    pic.desc.cr_qp_offset_delta = delta
    if int(pic.desc.n_coef_blocks):
        CR.make_conformant(pic, SC.make_conformant)
    return Stim(name, pic, frames_for(rng, "smooth" if delta else "noise"), (0, 0), checker)


@functools.lru_cache(maxsize=None)
def pictures():
    """the set, drawn once (the pictures are not to be changed)"""
    cur_p, cur_b = [0, 0], [0, 5]                # where `spread` stands in the P and in the B pictures
    out = [_plain("P %d" % n, n, (0, 16)[k & 1], cur_p, n_ref=n) for k, n in enumerate((16, 15, 9, 8, 5))]
    out += [
        _plain("P wp 16", 30, 16, cur_p, n_ref=16, wp="legal"),
        _plain("P dup 16", 31, 0, cur_p, n_ref=16, dup=True, frames="smooth", deblock_offsets=False, qp_mode=34),
        _plain("B 16+16", 40, 16, cur_b, deblock_offsets=False, qp_mode=34, b_picture=True, n_ref=16, n_ref_l1=16, weighted=False, cross=True, frames="smooth"),
        _plain("B implicit 16+16", 41, 0, cur_b, deblock_offsets=False, qp_mode=34, b_picture=True, n_ref=16, n_ref_l1=16, weighted=True, cross=True, frames="smooth"),
        _plain("B implicit 16+16 noise", 45, 16, cur_b, b_picture=True, n_ref=16, n_ref_l1=16, weighted=True),
        _plain("B wp 16+16", 42, 16, cur_b, deblock_offsets=False, qp_mode=34, b_picture=True, n_ref=16, n_ref_l1=16, wp="mild", cross=True, frames="smooth"),
        _plain("B 16+1", 43, 0, cur_b, b_picture=True, n_ref=16, n_ref_l1=1, weighted=True),
        _plain("B 1+16", 48, 16, cur_b, b_picture=True, n_ref=1, n_ref_l1=16, weighted=False),
        _plain("B implicit 9+7", 46, 0, cur_b, b_picture=True, n_ref=9, n_ref_l1=7, weighted=True),
        _plain("B wp 9+7", 47, 16, cur_b, b_picture=True, n_ref=9, n_ref_l1=7, wp="legal"),
        _high("P lists 16", 50, 0, "scaling", lists=61),
        _high("B lists 16+16", 51, 16, "scaling", b=True, lists=62),
        _high("P cr 16", 52, 16, "cr", cqo=3, delta=-13),
        _high("P t8 16", 53, 0, "t8x8", share=0.6),
        _high("B t8 16+16", 54, 16, "t8x8", b=True, share=0.6),
    ]
    assert len({st.name for st in out}) == len(out)
    return out


def by_name(name):
    return next(st for st in pictures() if st.name == name)


# ---- the expectation ---------------------------------------------------------------------------------------------------------------
def recon_for(st, slots=SLOTS):
    """a fresh model for the stimulus: tests/spec_recon.py for the set proper; the three pictures that are there for an instance are
    checked by the checker of what selects it"""
    if st.checker == "spec":
        return spec_recon.SpecRecon(W, H, slots)
    if st.checker == "t8x8":
        return T8.SpecRecon(W, H, slots)
    if st.checker == "scaling":
        return SC.SpecRecon(W, H, slots)
    assert st.checker == "cr", st.checker
    return CR.TwoChains(SC.SpecRecon, W, H, slots)


def decode(st, pic=None, frames=None, slots=SLOTS):
    model = recon_for(st, slots)
    for slot, f in (st.frames if frames is None else frames).items():
        model.store.write(slot, f)
    return [p.copy() for p in model.reconstruct(st.pic if pic is None else pic)]


def expected(st):
    return decode(st)


# ---- what the set reaches ----------------------------------------------------------------------------------------------------------
def used_entries(pic):
    """({entries of list 0}, {entries of list 1}) the inter macroblocks' quadrants use, as every road reads them"""
    out = (set(), set())
    for m in np.flatnonzero(pic.mb_records()["mb_type"] > N.MB_IPCM):
        for q in range(4):
            u0, u1, e0, e1 = IC.quadrant_lists(pic, int(m), q)
            if u0:
                out[0].add(e0)
            if u1:
                out[1].add(e1)
    return out


def assert_covered(stims):
    """AssertionError unless the pictures `stims`, as a SET, reach what the set is there for.  Returns the census."""
    c = IC.Census()
    for st in stims:
        IC.survey(st.pic, c)
        d = st.pic.desc
        assert int(d.mb_w) == W and int(d.mb_h) == H and int(d.dst_slot) in (0, SLOTS - 1)
        if st.checker == "spec":
            assert not RC.census(st.pic)[1], "%s: blocks out of range after make_conformant" % st.name
    coded, changed = sum(st.kept[0] for st in stims), sum(st.kept[1] for st in stims)
    assert changed <= coded // 2, "only %d of %d coded blocks kept the levels they were drawn with" % (coded - changed, coded)
    assert {int(st.pic.desc.dst_slot) for st in stims} == {0, SLOTS - 1}
    lengths = {(int(st.pic.desc.n_ref), int(st.pic.desc.n_ref_l1) if st.pic.desc.slice_type == N.SLICE_B else 0) for st in stims}
    assert lengths >= {(16, 0), (15, 0), (9, 0), (8, 0), (5, 0), (16, 16), (16, 1), (1, 16), (9, 7)}, sorted(lengths)
    for kind in ("mb", "quad"):
        for sl, lists in (("p", (0,)), ("b", (0, 1))):
            for l in lists:
                have = {k[1] for k in c.entries if k[0] == l and k[2] == kind and k[3] == sl}
                assert have == set(range(16)), "list %d, %s items of %s pictures: entries %s not used" % (l, kind, sl.upper(), sorted(set(range(16)) - have))
    # (explicit weights: every fetch is per block)
    for l in (0, 1):
        have = {k[1] for k in c.entries if k[0] == l and k[4] == "wp"}
        assert have == set(range(16)), "explicit weights, list %d: entries %s not used" % (l, sorted(set(range(16)) - have))
    bi = {k[:2] for k in c.pairs if k[2] == "quad"}
    high = {(a, b) for a, b in bi if a >= 8 and b >= 8}
    assert (15, 15) in high and {a for a, b in high} == set(range(8, 16)) == {b for a, b in high}, sorted(high)
    assert {(a, b) for a, b, kind, road in c.pairs if kind == "mb"} - {(a, a) for a in range(16)}
    generic = {k[1] for k in c.entries if k[4] == "generic"}
    assert any(e >= 8 for e in generic), "the generic two-list class without an index of 8 or more"
    assert any(a >= 8 and b >= 8 for a, b, kind, road in c.pairs if road == "generic")
    weighted = 0
    for st in stims:
        d = st.pic.desc
        if d.slice_type == N.SLICE_B and int(d.weighted_bipred) and not int(d.explicit_wp):
            pairs = {(a, b) for a, b in seam_fuzz.bi_pairs(st.pic) if a != b}
            weighted += len(pairs)
            same = [(a, b) for a, b in pairs if int(d.bipred_weight[a * 16 + b]) == int(d.bipred_weight[b * 16 + a])]
            assert not same, "%s: pairs %s weigh the same both ways round" % (st.name, same[:4])
    assert weighted >= 50, weighted
    dup = [st for st in stims if st.pic.desc.slice_type == N.SLICE_P and not int(st.pic.desc.explicit_wp)
           and len({int(st.pic.desc.ref_slot[i]) for i in DUP}) == 1 and used_entries(st.pic)[0] >= set(DUP)]
    assert dup, "no P picture names one slot at the indices %s" % (DUP,)
    assert {st.checker for st in stims} == {"spec", "scaling", "cr", "t8x8"}
    for st in stims:
        if st.checker == "t8x8":
            rec = st.pic.mb_records()
            assert ((rec["mb_type"] > N.MB_IPCM) & ((rec["intra_modes"] & N.MB_T8X8) != 0) & ((rec["coef_mask"] & 0xffff) != 0)).sum() >= 8, st.name
        if st.checker != "spec":
            assert all(e == set(range(16)) for e in used_entries(st.pic)[:2 if st.pic.desc.slice_type == N.SLICE_B else 1]), st.name
    return c


# ---- deliberately wrong copies of the reference ------------------------------------------------------------------------------------
def copy_picture(pic):
    """a picture of its own arrays with the same content"""
    new = seam_fuzz.SeamPicture(pic.mb_w, pic.mb_h)
    C.memmove(C.byref(new.desc), C.byref(pic.desc), C.sizeof(N.Picture))
    new.rec = pic.mb_records().copy()
    for name in ("mv", "ref_idx", "i4modes", "coefs", "mv_l1", "ref_idx_l1"):
        setattr(new, name, np.array(getattr(pic, name), copy=True))
    return new.seal()


def _is_b(pic):
    return pic.desc.slice_type == N.SLICE_B


def _low3(st):
    """(a) every reference index AND 7"""
    pic = copy_picture(st.pic)
    for a in (pic.ref_idx, pic.ref_idx_l1):
        a[:] = np.where(a >= 0, a & 7, a)
    return decode(st, pic)


def _uses_high(st):
    e0, e1 = used_entries(st.pic)
    return any(e >= 8 for e in e0 | e1)


def _l1_in_l0(st):
    """(b) list 1's index looked up in list 0's slots"""
    pic = copy_picture(st.pic)
    for i in range(N.MAX_REFS):
        pic.desc.ref_slot_l1[i] = pic.desc.ref_slot[i]
    return decode(st, pic)


def _uses_l1(st):
    d = st.pic.desc
    return _is_b(st.pic) and any(int(d.ref_slot_l1[e]) != int(d.ref_slot[e]) for e in used_entries(st.pic)[1])


def _weights_transposed(st):
    """(c) bipred_weight read at [r1 * 16 + r0]"""
    pic = copy_picture(st.pic)
    w = np.array(list(st.pic.desc.bipred_weight)).reshape(16, 16).T.reshape(-1)
    for i, v in enumerate(w):
        pic.desc.bipred_weight[i] = int(v)
    return decode(st, pic)


def _uses_implicit(st):
    d = st.pic.desc
    return _is_b(st.pic) and bool(int(d.weighted_bipred)) and not int(d.explicit_wp) and any(a != b for a, b in seam_fuzz.bi_pairs(st.pic))


def _wp_low3(st):
    """(d) explicit weights of entry `index & 7`"""
    pic = copy_picture(st.pic)
    t = np.ctypeslib.as_array(pic.desc.wp).reshape(2, 16, 3, 2)
    t[:, 8:] = t[:, :8].copy()
    return decode(st, pic)


def _uses_wp_high(st):
    return bool(int(st.pic.desc.explicit_wp)) and _uses_high(st)


def _by_index(st):
    """the picture with every (list, entry) naming a slot of its own that holds a copy of the entry's frame: motion compensation
    reads what it read, the reference PICTURES of any two (list, entry) differ"""
    pic = copy_picture(st.pic)
    d = pic.desc
    frames = dict(st.frames)
    at = SLOTS
    for n, slots in ((int(d.n_ref), d.ref_slot), (int(d.n_ref_l1) if _is_b(pic) else 0, d.ref_slot_l1)):
        for i in range(n):
            frames[at] = st.frames[int(slots[i])]
            slots[i] = at
            at += 1
    return pic, frames, at


def _strengths_by_index(st):
    """(e) boundary strengths from indices instead of pictures"""
    pic, frames, slots = _by_index(st)
    return decode(st, pic, frames, slots)


def strengths_differ(st):
    """the filtered edges of the picture whose strengths by picture and by index differ"""
    if not int(st.pic.desc.deblock):
        return 0
    other = _by_index(st)[0]
    rec, n = st.pic.mb_records(), 0
    for m in range(st.pic.n_mb):
        e = int(rec["edges"][m])
        for d in (0, 1):
            for edge in range(4):
                if not (e & N.EDGE_INNER if edge else e & (N.EDGE_LEFT if d == 0 else N.EDGE_TOP)):
                    continue
                n += DC.edge_strengths(st.pic, m, d, edge)[0] != DC.edge_strengths(other, m, d, edge)[0]
    return n


WRONG = collections.OrderedDict([
    ("index & 7", (_low3, _uses_high)),
    ("list 1 in list 0's slots", (_l1_in_l0, _uses_l1)),
    ("bipred_weight transposed", (_weights_transposed, _uses_implicit)),
    ("explicit weights of index & 7", (_wp_low3, _uses_wp_high)),
    ("strengths by index", (_strengths_by_index, lambda st: strengths_differ(st) > 0)),
])
# the pictures every wrong decoder must at least be tried on (the set's reason to hold them)
MUST_USE = {
    "index & 7": ["P 16", "P 15", "P 9", "P wp 16", "P dup 16", "B 16+16", "B 16+1", "B 1+16", "B implicit 9+7", "P lists 16", "B lists 16+16", "P cr 16", "P t8 16", "B t8 16+16"],
    "list 1 in list 0's slots": ["B 16+16", "B implicit 16+16", "B wp 16+16", "B 16+1", "B 1+16", "B implicit 9+7", "B lists 16+16", "B t8 16+16"],
    "bipred_weight transposed": ["B implicit 16+16", "B implicit 16+16 noise", "B implicit 9+7"],
    "explicit weights of index & 7": ["P wp 16", "B wp 16+16", "B wp 9+7"],
    "strengths by index": ["P dup 16", "B 16+16", "B implicit 16+16", "B wp 16+16"],
}
