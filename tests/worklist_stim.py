"""Directed pictures for the work lists of the motion-compensation stage (TEST INFRASTRUCTURE): pictures at the CPU->GPU seam whose
distribution of items over (band, key) is adversarial for the counting sort k_mc_sort* and the chunk walks of k_mc / k_mc_wp /
k_mc_second - every reachable key of every band populated and padded (the luma lists, and the chroma quadrant lists: one part-filled
chunk per key; chroma macroblock items: every key 1 modulo its chunk), 32 bands, one key holding everything, lists that are
empty inside a real launch.  Everything from seeds, drawn with inter_stim's Builder and seam_fuzz.make_picture; what each picture
asks of the lists is PROVED by tests/test_worklist_cpu.py with tests/worklist_model.py, not assumed here.

Geometries: WIDE 32 x 4 (band knob 0: four bands of 32 macroblocks - room for every key of a band at once) and DEEP 8 x 32 (band
knob 0: 32 bands of one row - MC_MAX_BANDS, every key slot of the sort's LDS arrays exists).

What the arithmetic of the lists allows (the reasons the CPU test's conditions are worded as they are):
* a whole macroblock is one YM and one CM item, a split one four YQ items and four CQ items.  28 whole macroblocks of a band are
  28 YM keys of one item and 28 CM items in four keys: `ym_each_key` makes them 17 + 1 + 9 + 1 (each = 1 modulo the chunk of 8).
* a P macroblock files all four quadrants, so a band's YQ items are a multiple of four and 30 keys of one item each cannot be:
  `yq_each_key` files 32 items, one key holds 3.  Its eight macroblocks' CQ entries (multiples of four, never = 1 modulo 32) lie
  in all four chroma keys, one part-filled chunk each.
* the generic two-list class files four quadrants per macroblock under at most two keys, and a bi-predicted quadrant files a first
  pass entry without residual: in `b_each_key` every key of YQ and CQ of both passes holds one part-filled chunk, the second
  pass's luma keys exactly one item."""
import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker as IC
from tests import inter_stim as S
from tests import seam_fuzz
from tests import worklist_model as M

WIDE, DEEP = (32, 4), (8, 32)
SLOTS = 3
B_WEIGHTS = S.B_WEIGHTS

# the 28 keys of an item with one vector: (key, phase class, clamped, coded) - neighbours differ in `clamped`, the last is the highest
Y28 = [(M.PC[pc] | (M.MCY_CLAMP if c else 0) | (M.MCY_RESID if r else 0), pc, bool(c), bool(r))
       for pc in IC.PHASE_CLASSES for r in (0, 1) for c in (0, 1)]
assert Y28[-1][0] == max(k[0] for k in Y28) and Y28[0][0] == 0
Y14 = {False: [k for k in Y28 if not k[3]], True: [k for k in Y28 if k[3]]}       # by coded


# ---- one macroblock ------------------------------------------------------------------------------------------------------------
def _vector(rng, b, m, blocks, kind, pc, clamp, far=False):
    """a vector of phase class pc for the item (its 4x4 blocks, raster) whose luma window lies inside the picture, or - clamp -
    reaches over the nearer vertical border: by one sample (the chroma window stays inside) or, far, by 6 .. 13 (chroma outside too)"""
    W, H = b.pic.mb_w * 16, b.pic.mb_h * 16
    n = IC.LUMA_WINDOW[kind][0]
    x0, y0 = (m % b.pic.mb_w) * 16 + (blocks[0] & 3) * 4, (m // b.pic.mb_w) * 16 + (blocks[0] >> 2) * 4
    frac = S.FRACTIONS[pc][int(rng.integers(0, len(S.FRACTIONS[pc])))]
    wx = int(np.clip(x0 - 2 + rng.integers(-24, 25), 0, W - n))
    wy = int(np.clip(y0 - 2 + rng.integers(-24, 25), 0, H - n))
    if clamp:
        past = int(rng.integers(6, 14)) if far else 1
        wx = -past if x0 < W // 2 else W - n + past
    return S.vector_onto(wx, wy, x0, y0, frac, False, rng)


def _code_luma(rng, b, m, raster_blocks):
    bb = raster_blocks[int(rng.integers(0, len(raster_blocks)))]
    b.levels[m][1 << S.DECODE_AT[(bb & 3, bb >> 2)]] = S.some_levels(rng)


def _code_chroma(rng, b, m):
    dc = np.zeros(16, np.int64)
    dc[:8] = rng.integers(-6, 7, size=8)
    dc[0] |= 1
    b.levels[m][N.COEF_CHROMA_DC] = dc
    b.levels[m][1 << int(rng.integers(16, 24))] = S.some_levels(rng, 15)


def _intra(b, m):
    r = b.pic.rec
    r["mb_type"][m], r["intra_modes"][m] = N.MB_I16x16, 2                   # Intra16x16 DC, chroma DC: legal everywhere
    b.pic.ref_idx[m * 4:m * 4 + 4] = -1
    b.pic.ref_idx_l1[m * 4:m * 4 + 4] = -1


def _lists(b, m, q, which, ref=0):
    """quadrant q (None: all four) predicts from 'l0', 'l1' or 'bi'"""
    sl = slice(m * 4, m * 4 + 4) if q is None else m * 4 + q
    b.pic.ref_idx[sl] = -1 if which == "l1" else ref
    b.pic.ref_idx_l1[sl] = -1 if which == "l0" else ref


def _whole(rng, b, m, key, far=False, cc=False, which="l0", key1=None):
    """one item: `key` = (_, phase class, clamped, coded) for the first pass's vector, key1 for list 1's of a 'bi' macroblock (its
    `coded` is the one that counts: the second pass adds the residual)"""
    blocks = tuple(range(16))
    mv1 = b.pic.mv_l1.reshape(-1, 16, 2)
    first = mv1 if which == "l1" else b.mv
    first[m] = _vector(rng, b, m, blocks, "mb", key[1], key[2], far)
    coded = key[3]
    if which == "bi":
        mv1[m] = _vector(rng, b, m, blocks, "mb", key1[1], key1[2], far)
        coded = key1[3]
    if b.pic.desc.slice_type == N.SLICE_B:
        _lists(b, m, None, which, int(rng.integers(0, 2)))
    if coded:
        _code_luma(rng, b, m, blocks)
    if cc:
        _code_chroma(rng, b, m)


def _quads(rng, b, m, spec, far=False, cc=False):
    """four quadrant items; spec[q] = (key, which, key1): key = (_, phase class or 'gen', clamped, coded) for the first pass's vector
    ('gen': the quadrant's 4x4 blocks differ), which = 'l0' / 'l1' / 'bi' (P pictures: 'l0'), key1 list 1's of a 'bi' quadrant"""
    is_b = b.pic.desc.slice_type == N.SLICE_B
    mv1 = b.pic.mv_l1.reshape(-1, 16, 2)
    if not is_b:
        b.pic.rec["mb_type"][m] = N.MB_P_8x8
    for q, (key, which, key1) in enumerate(spec):
        qb = IC.quad_blocks(q)
        first = mv1 if which == "l1" else b.mv
        coded = key[3]
        if key[1] == "gen":
            first[m, list(qb)] = _vector(rng, b, m, qb, "quad", "copy", False)
            first[m, qb[3]] += (4, 0)
        else:
            first[m, list(qb)] = _vector(rng, b, m, qb, "quad", key[1], key[2], far)
        if which == "bi":
            mv1[m, list(qb)] = _vector(rng, b, m, qb, "quad", key1[1], key1[2], far)
            coded = key1[3]
        if is_b:
            _lists(b, m, q, which, int(rng.integers(0, 2)))
        if coded:
            _code_luma(rng, b, m, qb)
    if cc:
        _code_chroma(rng, b, m)


def _generic(rng, b, m, coded_quadrant=None, cc=False):
    """a bi-predicted macroblock whose vectors differ inside every quadrant: the generic two-list class"""
    mv1 = b.pic.mv_l1.reshape(-1, 16, 2)
    b.mv[m] = rng.integers(-30, 31, size=(16, 2))
    mv1[m] = rng.integers(-30, 31, size=(16, 2))
    for q in range(4):
        qb = IC.quad_blocks(q)
        if len({tuple(v) for v in b.mv[m, list(qb)].tolist()}) == 1:
            b.mv[m, qb[3]] += (4, 0)
    _lists(b, m, None, "bi", int(rng.integers(0, 2)))
    if coded_quadrant is not None:
        _code_luma(rng, b, m, IC.quad_blocks(coded_quadrant))
    if cc:
        _code_chroma(rng, b, m)


GEN = {False: (M.PC_GEN | M.MCY_CLAMP, "gen", True, False), True: (M.PC_GEN | M.MCY_CLAMP | M.MCY_RESID, "gen", True, True)}


def _p_path_gen(rng, b, m, k2, k3, cc=False):
    """a macroblock on the one-list road (P picture, or list 0 only in a B picture): quadrants 0 and 1 with differing vectors, not
    coded / coded (PC_GEN | MCY_CLAMP, ... | MCY_RESID: the chroma key is clamped), quadrants 2 and 3 with the keys k2, k3"""
    _quads(rng, b, m, [(GEN[False], "l0", None), (GEN[True], "l0", None), (k2, "l0", None), (k3, "l0", None)], cc=cc)


def _builder(geom, b_picture=False, weighted=False):
    b = S.Builder(geom[0], geom[1], b_picture=b_picture, qp=26)
    if b_picture and weighted:
        b.pic.desc.weighted_bipred = 1
        for e0 in range(2):
            for e1 in range(2):
                b.pic.desc.bipred_weight[e0 * N.MAX_REFS + e1] = B_WEIGHTS[e0 * 2 + e1]
    return b


def _finish(name, rng, b, used):
    """every macroblock not in `used` becomes intra; frames for slots 1 and 2"""
    for m in range(b.pic.n_mb):
        if m not in used:
            _intra(b, m)
    return S.stim(name, b.finish(), S.frames_for(rng, b.pic.mb_w, b.pic.mb_h))


# ---- every key of every band ---------------------------------------------------------------------------------------------------
def ym_each_key(seed=9101):
    rng = np.random.default_rng(seed)
    b, used = _builder(WIDE), set()
    for band in range(WIDE[1]):
        clamped_seen = cc_given = 0
        for i, key in enumerate(Y28):
            m = band * WIDE[0] + 2 + i                           # (columns 2 .. 29)
            far = cc = False
            if key[2] and clamped_seen < 2:                      # CM keys CLAMP and CLAMP | RESID: one macroblock each
                far, cc = True, clamped_seen == 1
                clamped_seen += 1
            elif cc_given < 9:                                   # CM key RESID: nine; the remaining seventeen: key 0
                cc, cc_given = True, cc_given + 1
            _whole(rng, b, m, key, far=far, cc=cc)
            b.pic.ref_idx[m * 4:m * 4 + 4] = int(rng.integers(0, 2))
            used.add(m)
    return _finish("ym_each_key", rng, b, used)


def yq_each_key(seed=9102):
    rng = np.random.default_rng(seed)
    b, used = _builder(WIDE), set()
    for band in range(WIDE[1]):
        m0 = band * WIDE[0] + 3 + band                           # eight macroblocks, two columns apart
        keys = Y28 + [Y28[0], Y28[0]]                            # (30 one-vector slots for 28 keys: key 0 holds three)
        _p_path_gen(rng, b, m0, keys[28], keys[29])
        used.add(m0)
        for j in range(7):
            m = m0 + 2 * (j + 1)
            # CQ keys: the macroblock above CLAMP, then CLAMP | RESID, RESID, and five of key 0
            _quads(rng, b, m, [(k, "l0", None) for k in keys[4 * j:4 * j + 4]], far=j == 0, cc=j in (0, 1))
            b.pic.ref_idx[m * 4:m * 4 + 4] = rng.integers(0, 2, size=4)
            used.add(m)
    return _finish("yq_each_key", rng, b, used)


def b_each_key(seed=9103):
    rng = np.random.default_rng(seed)
    b, used = _builder(WIDE, b_picture=True, weighted=True), set()
    for band in range(WIDE[1]):
        m0 = band * WIDE[0] + 1
        for j in range(14):
            # quadrants 0 / 1 predict from one list (list 0, list 1), coded: the RESID keys of the first pass; 2 / 3 from both: their
            # first-pass entries carry Z (the keys without RESID), their second-pass entries all 28 keys once; the second pass's
            # chroma entries of quadrants 0 / 1 are carried (MCE_KEEP)
            spec = [(Y14[True][(2 * j) % 14], "l0", None), (Y14[True][(2 * j + 1) % 14], "l1", None),
                    (Y14[False][(2 * j) % 14], "bi", Y28[2 * j]), (Y14[False][(2 * j + 1) % 14], "bi", Y28[2 * j + 1])]
            # chroma keys of both passes: 0, CLAMP, RESID, CLAMP | RESID in turn - 4 / 4 / 3 / 3 macroblocks (with the one-list
            # macroblock below: five under CLAMP in the first pass), every key less than one chunk of 32 entries
            _quads(rng, b, m0 + j, spec, far=bool(j & 1), cc=bool(j & 2))
            used.add(m0 + j)
        _p_path_gen(rng, b, m0 + 15, Y14[False][0], Y14[True][0])
        _lists(b, m0 + 15, None, "l0", 1)
        _generic(rng, b, m0 + 17, coded_quadrant=band, cc=False)
        _generic(rng, b, m0 + 19, coded_quadrant=None, cc=True)
        used |= {m0 + 15, m0 + 17, m0 + 19}
    return _finish("b_each_key", rng, b, used)


# ---- 32 bands ------------------------------------------------------------------------------------------------------------------
def deep_last_slot(b_picture, seed=9104):
    """DEEP: keys rotate over the bands; the last band holds the highest key of every list (both passes of the B picture)"""
    rng = np.random.default_rng(seed + int(b_picture))
    w, h = DEEP
    b, used = _builder(DEEP, b_picture=b_picture, weighted=True), set()
    top, top_nr = Y28[-1], Y14[False][-1]
    for band in range(h):
        last = band == h - 1
        m0 = band * w
        rot = lambda k: Y28[(band * 4 + k) % 28]
        if not b_picture:
            for i in range(4):                                   # four whole macroblocks, three split ones, one intra
                key = top if last and i == 0 else rot(i)
                _whole(rng, b, m0 + i, key, far=(last and i == 0) or bool((band + i) & 1), cc=(last and i == 0) or (band + i) % 3 == 0)
            _p_path_gen(rng, b, m0 + 4, rot(5), rot(6), cc=last or bool(band & 1))
            for i in (5, 6):
                _quads(rng, b, m0 + i, [(Y28[(band * 8 + (i - 5) * 4 + q) % 28], "l0", None) for q in range(4)], far=bool(band & 2), cc=bool((band + i) & 1))
                b.pic.ref_idx[(m0 + i) * 4:(m0 + i) * 4 + 4] = rng.integers(0, 2, size=4)
            used |= set(range(m0, m0 + 7))
            continue
        # B: a one-list whole macroblock, a bi-predicted whole one, two split ones with carried quadrants, one on the one-list road
        # with differing vectors, one generic, two intra
        _whole(rng, b, m0, top if last else Y28[band % 28], far=last or bool(band & 1), cc=last or band % 3 == 0, which="l1" if band & 1 else "l0")
        _whole(rng, b, m0 + 1, Y14[False][band % 14], far=last or bool(band & 2), cc=last or band % 3 == 1, which="bi", key1=top if last else Y28[(band + 5) % 28])
        for i in (2, 3):
            k = band * 4 + (i - 2) * 2
            spec = [(Y28[k % 28], "l0", None), (Y28[(k + 1) % 28], "l1", None),
                    (Y14[False][k % 14], "bi", top if last and i == 2 else Y28[(k + 7) % 28]), (Y14[False][(k + 1) % 14], "bi", Y28[(k + 8) % 28])]
            _quads(rng, b, m0 + i, spec, far=(last and i == 2) or bool((band + i) & 2), cc=(last and i == 2) or bool((band + i) & 1))
        _p_path_gen(rng, b, m0 + 4, rot(2), rot(3), cc=bool(band & 1))
        _lists(b, m0 + 4, None, "l0", 0)
        _generic(rng, b, m0 + 5, coded_quadrant=band % 4 if band % 5 else None, cc=last or bool(band & 1))
        used |= set(range(m0, m0 + 6))
    return _finish("deep_last_slot %s" % ("B" if b_picture else "P"), rng, b, used)


# ---- one key, no key, one item -------------------------------------------------------------------------------------------------
def one_key(geom, pulled_in=True, seed=9105):
    """every macroblock P_SKIP-like: one reference, no levels, vector 0.  With vector 0 the window of a macroblock on the picture's
    border reaches over it (21 x 21 from two samples outside the macroblock) - a second key, `all_skip`; pulled_in moves those windows
    inside by whole samples, and ONE key of YM and of CM holds every item of a band - `one_key`"""
    rng = np.random.default_rng(seed + geom[0] + 2 * int(pulled_in))
    w, h = geom
    b = _builder(geom)
    for m in range(w * h):
        b.pic.rec["mb_type"][m] = N.MB_P_SKIP
        if pulled_in:
            x, y = m % w, m // w
            b.mv[m] = (4 * (2 if x == 0 else -3 if x == w - 1 else 0), 4 * (2 if y == 0 else -3 if y == h - 1 else 0))
    return _finish("%s %dx%d" % ("one_key" if pulled_in else "all_skip", w, h), rng, b, set(range(w * h)))


def one_key_wp(seed=9106):
    rng = np.random.default_rng(seed)
    pic = seam_fuzz.make_picture(rng, WIDE[0], WIDE[1], n_ref=2, slots=SLOTS, dst_slot=0, level_style="small", qp_mode="random", intra_share=0.0,
                                 explicit_wp="legal")
    return S.stim("one_key_wp", pic, S.frames_for(rng, *WIDE))


def empty(geom, seed=9107):
    """a P picture of intra macroblocks only (drawn: both intra types, levels)"""
    rng = np.random.default_rng(seed + geom[0])
    pic = seam_fuzz.make_picture(rng, geom[0], geom[1], n_ref=2, slots=SLOTS, dst_slot=0, level_style="small", qp_mode="random", intra_share=2.0)
    return S.stim("empty %dx%d" % geom, pic, S.frames_for(rng, *geom))


SINGLES = ("tl", "tr", "bl", "br", "mid")


def single(where, geom=DEEP, seed=9108):
    """exactly one inter macroblock, with a residual: in a corner one whole item (one YM, one CM entry), in the middle four quadrant
    items under one key (YQ, CQ)"""
    rng = np.random.default_rng(seed + SINGLES.index(where) + geom[0])
    w, h = geom
    m = {"tl": 0, "tr": w - 1, "bl": (h - 1) * w, "br": w * h - 1, "mid": (h // 2) * w + w // 2}[where]
    b = _builder(geom)
    if where == "mid":
        key = next(k for k in Y28 if k[1] == "diag" and k[3] and not k[2])
        _quads(rng, b, m, [(key, "l0", None)] * 4, cc=True)       # four coded quadrants inside the picture, one phase class ...
        b.pic.ref_idx[m * 4:m * 4 + 4] = (0, 1, 0, 1)             # ... two references: four items, one key
    else:
        _whole(rng, b, m, Y28[-1], far=True, cc=True)
    return _finish("single_%s %dx%d" % ((where,) + geom), rng, b, {m})


# ---- the second pass of a B picture --------------------------------------------------------------------------------------------
def b_second(full, seed=9109):
    """B pictures whose second-pass lists are empty (no quadrant predicts from both lists) or as long as the first pass's (every
    quadrant does; every item coded, so each pass files a band's items under as many keys)"""
    rng = np.random.default_rng(seed + int(full))
    b = _builder(WIDE, b_picture=True, weighted=True)
    n = WIDE[0] * WIDE[1]
    for m in range(n):
        k0, k1 = Y14[False][(m % 7) * 2], Y14[True][((m + 3) % 7) * 2]         # (inside the picture, every phase class)
        assert not k0[2] and not k1[2]
        if full:
            if m & 1:
                _quads(rng, b, m, [(k0, "bi", k1)] * 4, cc=True)
            else:
                _whole(rng, b, m, k0, cc=True, which="bi", key1=k1)
        elif m & 1:
            _quads(rng, b, m, [(Y28[(m + q) % 28], "l1" if (m + q) & 2 else "l0", None) for q in range(4)], cc=bool(m & 2))
        else:
            _whole(rng, b, m, Y28[m % 28], cc=bool(m & 4), which="l1" if m & 2 else "l0")
    return _finish("b_second_%s" % ("full" if full else "empty"), rng, b, set(range(n)))


# ---- ordinary pictures: the successors whose lists would take the damage ---------------------------------------------------------
def ordinary(geom, b_picture, k, seed=9110):
    rng = np.random.default_rng(seed + 100 * geom[0] + 10 * int(b_picture) + k)
    pic = seam_fuzz.make_picture(rng, geom[0], geom[1], n_ref=2, slots=SLOTS, dst_slot=0, level_style="small", qp_mode="random", b_picture=b_picture,
                                 n_ref_l1=2)
    return S.stim("ordinary %s %dx%d #%d" % (("B" if b_picture else "P",) + geom + (k,)), pic, S.frames_for(rng, *geom))


def all_stims():
    """{name: Stim} of every directed picture (the ordinary ones are drawn where they are used)"""
    out = [ym_each_key(), yq_each_key(), b_each_key(), deep_last_slot(False), deep_last_slot(True), one_key_wp(), b_second(False), b_second(True)]
    for geom in (WIDE, DEEP):
        out += [one_key(geom), one_key(geom, pulled_in=False), empty(geom), single("mid", geom)]
    out += [single(where) for where in SINGLES if where != "mid"]
    return {st.name: st for st in out}
