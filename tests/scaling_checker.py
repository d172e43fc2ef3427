"""Checker for pictures with scaling matrices (TEST INFRASTRUCTURE), written from the text of H.264 - 7.3.2.1.1.1 / 7.4.2.1.1 and
table 7-2 (the syntax of a list, its default and its fall-back rules), tables 7-3 / 7-4 (the default lists), 8.5.6 (weightScale is
the list put through the inverse frame zig-zag), 8.5.9 (LevelScale = weightScale * normAdjust) and the scaling formulas of 8.5.10
(Intra16x16 luma DC), 8.5.11 (chroma DC), 8.5.12.1 (4x4 blocks) and 8.5.13 (8x8 blocks) - not from kernel_scaling.h, and not from
the reference, whose decoder forces flat lists.  Python integers of unbounded size.

The scans and the transforms are residual_checker's and t8x8_checker's, by import; what is new here is the scaling with the list of
the block: 0 / 1 / 2 Intra Y / Cb / Cr, 3 / 4 / 5 Inter Y / Cb / Cr (4x4), 6 / 7 Intra / Inter Y (8x8).  Intra or inter is the
macroblock's.  A picture's lists are its descriptor's (include/p264hip.h: scaling_lists, scaling4x4, scaling8x8 - resolved, in scan
order); a descriptor with scaling_lists = 0 means every weight 16, and then everything here equals residual_checker / t8x8_checker
value for value (tests/test_scaling_cpu.py).

Range: as in residual_checker - every value the standard bounds is recorded in a `Range`, and a macroblock with a value outside
-2^15 .. 2^15 - 1 has no defined result (OutOfRange).  `make_conformant` shrinks the levels of the blocks that feed such a value.

`Census` records what the scaled blocks exercised (tests/scaling_stim.py: assert_covered).  `SpecRecon` is i8x8_checker.SpecRecon
with every residual taken from here."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import i8x8_checker as I8
from tests import inter_checker, residual_checker as RC, spec_recon
from tests import t8x8_checker as T8
from tests.residual_checker import OutOfRange, Range

# tables 7-3 and 7-4, in scan order
DEFAULT_4X4_INTRA = [6, 13, 13, 20, 20, 20, 28, 28, 28, 28, 32, 32, 32, 37, 37, 42]
DEFAULT_4X4_INTER = [10, 14, 14, 20, 20, 20, 24, 24, 24, 24, 27, 27, 27, 30, 30, 34]
DEFAULT_8X8_INTRA = [6, 10, 10, 13, 11, 13, 16, 16, 16, 16, 18, 18, 18, 18, 18, 23, 23, 23, 23, 23, 23, 25, 25, 25, 25, 25, 25, 25, 27, 27, 27, 27, 27, 27, 27, 27,
                     29, 29, 29, 29, 29, 29, 29, 31, 31, 31, 31, 31, 31, 33, 33, 33, 33, 33, 36, 36, 36, 36, 38, 38, 38, 40, 40, 42]
DEFAULT_8X8_INTER = [9, 13, 13, 15, 13, 15, 17, 17, 17, 17, 19, 19, 19, 19, 19, 21, 21, 21, 21, 21, 21, 22, 22, 22, 22, 22, 22, 22, 24, 24, 24, 24, 24, 24, 24, 24,
                     25, 25, 25, 25, 25, 25, 25, 27, 27, 27, 27, 27, 27, 28, 28, 28, 28, 28, 30, 30, 30, 30, 32, 32, 32, 33, 33, 35]
DEFAULTS = [DEFAULT_4X4_INTRA] * 3 + [DEFAULT_4X4_INTER] * 3 + [DEFAULT_8X8_INTRA, DEFAULT_8X8_INTER]
FLAT = [[16] * 16] * 6 + [[16] * 64] * 2
SIZES = [16] * 6 + [64] * 2
INTRA_Y, INTRA_CB, INTRA_CR, INTER_Y, INTER_CB, INTER_CR, INTRA_Y8, INTER_Y8 = range(8)


# ---- 7.3.2.1.1.1, 7.4.2.1.1, table 7-2: the lists of a parameter set ----------------------------------------------------------------
def parse_list(deltas, size):
    """scaling_list( ): the delta_scale values read (a list ends early when a nextScale is 0) -> (the list, useDefaultScalingMatrixFlag,
    how many deltas were consumed)"""
    out, last, nxt, used, use_default = [0] * size, 8, 8, 0, False
    for j in range(size):
        if nxt != 0:
            nxt = (last + deltas[used] + 256) % 256
            used += 1
            use_default = j == 0 and nxt == 0
        out[j] = last if nxt == 0 else nxt
        last = out[j]
    return out, use_default, used


def deltas_of(lst, stop_early=True):
    """the shortest delta_scale sequence that codes the list (stop_early: a tail that repeats its last value is cut by one delta that
    makes nextScale 0)"""
    n = len(lst)
    end = n
    if stop_early:
        while end > 1 and lst[end - 1] == lst[end - 2]:
            end -= 1
    out, last = [], 8
    for j in range(end):
        d = (lst[j] - last + 128) % 256 - 128
        out.append(d)
        last = lst[j]
    if end < n:
        out.append((0 - last + 128) % 256 - 128)
    return out


def resolve(coded, fallback=None):
    """table 7-2.  coded[n]: None (list n not present), "default" (useDefaultScalingMatrixFlag) or the list as coded, n = 0 .. 7 (a
    PPS without transform_8x8_mode_flag codes six: 6 and 7 count as not present).  fallback: None - rule A (sets the SPS carries, and
    a PPS's when the SPS has no matrix); the SPS's eight resolved lists - rule B."""
    coded = list(coded) + [None] * (8 - len(coded))
    out = []
    for n in range(8):
        c = coded[n]
        if c is None:
            if n in (0, 3, 6, 7):
                out.append(list(DEFAULTS[n] if fallback is None else fallback[n]))
            else:
                out.append(list(out[n - 1]))
        elif isinstance(c, str):
            out.append(list(DEFAULTS[n]))
        else:
            assert len(c) == SIZES[n]
            out.append([int(v) for v in c])
    return out


def picture_lists(sps=None, pps=None):
    """the eight lists of a picture: sps / pps = coded[] of the set's matrix, None where the set carries none"""
    if sps is None and pps is None:
        return [list(x) for x in FLAT]
    seq = resolve(sps) if sps is not None else None
    if pps is None:
        return seq
    return resolve(pps, seq)


# ---- the descriptor ------------------------------------------------------------------------------------------------------------
def lists_of(pic):
    """the eight lists of a picture at the seam, scan order; flat where the descriptor says 0"""
    d = pic.desc
    if not int(d.scaling_lists):
        return [list(x) for x in FLAT]
    return [[int(d.scaling4x4[n * 16 + k]) for k in range(16)] for n in range(6)] + [[int(d.scaling8x8[n * 64 + k]) for k in range(64)] for n in range(2)]


def set_lists(pic, lists, flag=1):
    d = pic.desc
    d.scaling_lists = flag
    for n in range(6):
        for k in range(16):
            d.scaling4x4[n * 16 + k] = int(lists[n][k])
    for n in range(2):
        for k in range(64):
            d.scaling8x8[n * 64 + k] = int(lists[6 + n][k])


def table_bytes(lists):
    return bytes(int(v) for lst in lists for v in lst)


def weight4(lst):
    """8.5.6: the list through the inverse 4x4 frame scan -> weightScale4x4[i][j]"""
    w = [[0] * 4 for _ in range(4)]
    for k, (i, j) in enumerate(RC.ZIGZAG):
        w[i][j] = int(lst[k])
    return w


def weight8(lst):
    w = [[0] * 8 for _ in range(8)]
    for k in range(64):
        w[T8.SCAN8[k] >> 3][T8.SCAN8[k] & 7] = int(lst[k])
    return w


def norm4(m, i, j):
    """normAdjust4x4 (8-315)"""
    return RC.V[m][0] if i % 2 == 0 and j % 2 == 0 else RC.V[m][1] if i % 2 == 1 and j % 2 == 1 else RC.V[m][2]


def norm8(m, i, j):
    return T8.V8[m][T8.CLASS8[(i & 3) * 4 + (j & 3)]]


class Census:
    """what the scaled blocks exercised: lists[n] - non-zero levels of list n met at a position whose weight is not 16; branches -
    (rule, "shift" / "round", qP) of blocks with a non-zero level; chroma_dc - (plane, "intra" / "inter") with a non-zero level;
    classes[(n, class)] - non-zero levels of list n met at a weight of that class (weight_class: 0, 1 .. 3, 4 .. 64, 65 .. 255), the DC
    blocks among them also in dc_classes[("luma", class)] (Intra16x16) and dc_classes[((plane, "intra" / "inter"), class)] (chroma)"""

    def __init__(self):
        self.lists = collections.Counter()
        self.branches = collections.Counter()
        self.chroma_dc = collections.Counter()
        self.classes = collections.Counter()
        self.dc_classes = collections.Counter()


WEIGHT_CLASSES = ("0", "1..3", "4..64", "65..255")


def weight_class(w):
    """a byte of a list -> one of WEIGHT_CLASSES (4 .. 64 is what every list before tests/scaling_stim.py: extreme_set held)"""
    assert 0 <= w <= 255
    return WEIGHT_CLASSES[0 if w == 0 else 1 if w <= 3 else 2 if w <= 64 else 3]


# ---- the formulas --------------------------------------------------------------------------------------------------------------
def scale4x4(c, qp, w, rng, dc=None, census=None, n=None):
    """8.5.12.1 with LevelScale4x4(m, i, j) = w[i][j] * normAdjust4x4(m, i, j); dc: the already scaled d00"""
    m, s = qp % 6, qp // 6
    d = [[0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            ls = w[i][j] * norm4(m, i, j)
            if dc is not None and i == 0 and j == 0:
                d[i][j] = dc
                continue
            if qp >= 24:
                d[i][j] = (c[i][j] * ls) << (s - 4)
            else:
                d[i][j] = (c[i][j] * ls + (1 << (3 - s))) >> (4 - s)
            if census is not None and c[i][j]:
                census.branches[("4x4", "shift" if qp >= 24 else "round", qp)] += 1
                census.classes[(n, weight_class(w[i][j]))] += 1
                if w[i][j] != 16:
                    census.lists[n] += 1
    rng.see("d", [x for r in d for x in r])
    return d


def luma_dc(c, qp, w, rng, census=None):
    """8.5.10 with LevelScale4x4(qP % 6, 0, 0) of the Intra Y list"""
    f = RC.luma_dc_transform(c, rng)
    ls = w[0][0] * norm4(qp % 6, 0, 0)
    if qp >= 36:
        dc = [[(x * ls) << (qp // 6 - 6) for x in r] for r in f]
    else:
        dc = [[(x * ls + (1 << (5 - qp // 6))) >> (6 - qp // 6) for x in r] for r in f]
    if census is not None and any(x for r in f for x in r):
        census.branches[("luma dc", "shift" if qp >= 36 else "round", qp)] += 1
        census.classes[(INTRA_Y, weight_class(w[0][0]))] += 1
        census.dc_classes[("luma", weight_class(w[0][0]))] += 1
        if w[0][0] != 16:
            census.lists[INTRA_Y] += 1
    rng.see("dcY", [x for r in dc for x in r])
    return dc


def chroma_dc(c4, qpc, w, rng, census=None, n=None):
    """8.5.11 with LevelScale4x4(QP'c % 6, 0, 0) of the plane's own list"""
    c = [[int(c4[0]), int(c4[1])], [int(c4[2]), int(c4[3])]]
    f = [[c[0][0] + c[0][1] + c[1][0] + c[1][1], c[0][0] - c[0][1] + c[1][0] - c[1][1]],
         [c[0][0] + c[0][1] - c[1][0] - c[1][1], c[0][0] - c[0][1] - c[1][0] + c[1][1]]]
    rng.see("chroma DC f", [x for r in f for x in r])
    ls = w[0][0] * norm4(qpc % 6, 0, 0)
    dc = [((x * ls) << (qpc // 6)) >> 5 for r in f for x in r]
    if census is not None and any(x for r in f for x in r):
        which = (1 if n in (INTRA_CB, INTER_CB) else 2, "intra" if n < 3 else "inter")
        census.chroma_dc[which] += 1
        census.classes[(n, weight_class(w[0][0]))] += 1
        census.dc_classes[(which, weight_class(w[0][0]))] += 1
        if w[0][0] != 16:
            census.lists[n] += 1
    rng.see("dcC", dc)
    return dc


def scale8x8(c, qp, w, rng, census=None, n=None):
    """8.5.13 with LevelScale8x8(m, i, j) = w[i][j] * normAdjust8x8(m, i, j)"""
    m, s = qp % 6, qp // 6
    if qp >= 36:
        d = [[(c[i][j] * w[i][j] * norm8(m, i, j)) << (s - 6) for j in range(8)] for i in range(8)]
    else:
        d = [[(c[i][j] * w[i][j] * norm8(m, i, j) + (1 << (5 - s))) >> (6 - s) for j in range(8)] for i in range(8)]
    if census is not None:
        for i in range(8):
            for j in range(8):
                if c[i][j]:
                    census.branches[("8x8", "shift" if qp >= 36 else "round", qp)] += 1
                    census.classes[(n, weight_class(w[i][j]))] += 1
                    if w[i][j] != 16:
                        census.lists[n] += 1
    rng.see("d", [x for r in d for x in r])
    return d


def block4x4(levels, qp, w, rng, ac_only=False, dc=None, census=None, n=None):
    return RC.transform4x4(scale4x4(RC.unscan(levels, ac_only), qp, w, rng, dc, census, n), rng)


def block8x8(levels, qp, w, rng, census=None, n=None):
    return T8.transform8x8(scale8x8(T8.unscan8(levels), qp, w, rng, census, n), rng)


# ---- a macroblock ---------------------------------------------------------------------------------------------------------------
def is_8x8(r):
    return bool(int(r["intra_modes"]) & (N.MB_T8X8 if int(r["mb_type"]) > N.MB_IPCM else N.MB_I8X8))


def residual_of(pic, m, refuse=True, census=None, lists=None):
    """residual_checker.residual_of with the picture's lists and with the 8x8 blocks of flagged records: ({(plane, x, y): r[4][4] or
    r[8][8]} - 8x8 luma blocks at their quadrant's place -, the Range, {blame key: names} per level block that fed a value out of
    range; blame key: a coef_mask bit / COEF_*_DC for a 4x4 entry, ("8x8", k) for the four entries of 8x8 block k)"""
    r = pic.mb_records()[m]
    mask, qp, t = int(r["coef_mask"]), int(r["qp"]), int(r["mb_type"])
    assert t != N.MB_IPCM
    lists = lists_of(pic) if lists is None else lists
    intra = t <= N.MB_IPCM
    out, total, blame = {}, Range(), {}

    def run(bits, fn):
        rng = Range()
        v = fn(rng)
        total.n += rng.n
        total.bad += rng.bad
        if rng.bad:
            for b in bits:
                blame.setdefault(b, []).extend(rng.bad)
        return v
    ny = INTRA_Y if intra else INTER_Y
    wy = weight4(lists[ny])
    if is_8x8(r):
        (I8 if intra else T8).check_record(r)
        n8 = INTRA_Y8 if intra else INTER_Y8
        w8 = weight8(lists[n8])
        for k in range(4):
            if mask >> (4 * k) & 1:
                out[(0, (k & 1) * 8, (k >> 1) * 8)] = run([("8x8", k)], lambda g: block8x8(T8.levels8_of(pic, r, k), qp, w8, g, census, n8))
    elif t == N.MB_I16x16:
        dc = [[0] * 4 for _ in range(4)]
        if mask & N.COEF_LUMA_DC:
            dc = run([N.COEF_LUMA_DC], lambda g: luma_dc(RC.unscan(RC.levels_of(pic, r, N.COEF_LUMA_DC)), qp, wy, g, census))
        for i in range(16):
            lv = RC.levels_of(pic, r, 1 << i) if mask >> i & 1 else [0] * 16
            bits = ([1 << i] if mask >> i & 1 else []) + ([N.COEF_LUMA_DC] if mask & N.COEF_LUMA_DC else [])
            out[(0, RC.BLK_X[i] * 4, RC.BLK_Y[i] * 4)] = run(bits, lambda g: block4x4(lv, qp, wy, g, True, dc[RC.BLK_Y[i]][RC.BLK_X[i]], census, ny))
    else:
        for i in range(16):
            if mask >> i & 1:
                out[(0, RC.BLK_X[i] * 4, RC.BLK_Y[i] * 4)] = run([1 << i], lambda g: block4x4(RC.levels_of(pic, r, 1 << i), qp, wy, g, census=census, n=ny))
    if int(r["cbp"]) >> 4:
        qpc = RC.chroma_qp(qp, int(pic.desc.chroma_qp_offset))
        for ch in range(2):
            nc = (INTRA_CB if intra else INTER_CB) + ch
            wc = weight4(lists[nc])
            has_dc = bool(mask & N.COEF_CHROMA_DC)
            dc = [0] * 4
            if has_dc:
                dc = run([N.COEF_CHROMA_DC], lambda g: chroma_dc(RC.levels_of(pic, r, N.COEF_CHROMA_DC)[ch * 4:ch * 4 + 4], qpc, wc, g, census, nc))
            for i in range(4):
                b = 16 + ch * 4 + i
                lv = RC.levels_of(pic, r, 1 << b) if mask >> b & 1 else [0] * 16
                bits = ([1 << b] if mask >> b & 1 else []) + ([N.COEF_CHROMA_DC] if has_dc else [])
                out[(1 + ch, (i & 1) * 4, (i >> 1) * 4)] = run(bits, lambda g: block4x4(lv, qpc, wc, g, True, dc[i], census, nc))
    else:
        assert not mask & (0x00ff0000 | N.COEF_CHROMA_DC), "macroblock %d: chroma levels in the mask, none in cbp" % m
    if refuse and not total.ok:
        raise OutOfRange("macroblock %d: %s outside -2^15 .. 2^15 - 1: H.264 defines no result" % (m, sorted(set(total.bad))))
    return out, total, blame


def construct(plane, x, y, r):
    """8.5.14 for a block of any size"""
    for i in range(len(r)):
        for j in range(len(r[i])):
            plane[y + i, x + j] = min(max(int(plane[y + i, x + j]) + r[i][j], 0), 255)


def add_residual(pic, m, F, census=None):
    d = pic.desc
    x0, y0 = (m % d.mb_w) * 16, (m // d.mb_w) * 16
    for (plane, x, y), r in residual_of(pic, m, census=census)[0].items():
        construct(F[plane], (x0 >> (plane > 0)) + x, (y0 >> (plane > 0)) + y, r)


def luma8x8_of(pic, m, refuse=True):
    """i8x8_checker.luma8x8_of / t8x8_checker.luma8x8_of with the picture's lists"""
    out, rng, _ = residual_of(pic, m, refuse)
    return {(x >> 3) + 2 * (y >> 3): r for (plane, x, y), r in out.items() if plane == 0}, rng


def chroma_residual_of(pic, m):
    return {k: v for k, v in residual_of(pic, m)[0].items() if k[0]}


def census(pic, sink=None):
    """(coded level blocks of the picture, {(macroblock, blame key): names} of those that feed a value out of range); sink: a Census
    that sees every block"""
    rec = pic.mb_records()
    lists = lists_of(pic)
    n, flagged = 0, {}
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) == N.MB_IPCM:
            continue
        mask = int(rec["coef_mask"][m])
        n += bin(mask & 0x03ffffff).count("1")
        if mask:
            for key, names in residual_of(pic, m, refuse=False, census=sink, lists=lists)[2].items():
                flagged[(m, key)] = names
    return n, flagged


def make_conformant(pic, max_rounds=60):
    """residual_checker.make_conformant for a picture with lists and with 8x8 blocks: the levels of every block that feeds a value out
    of range are halved (the last non-zero level never below magnitude 1; where nothing is left to halve the macroblock's QP goes down by 6: a
    weight of 64 is two QP periods) until the census is clean.  Returns (coded entries, blocks
    changed)."""
    changed = set()
    for _ in range(max_rounds):
        n, flagged = census(pic)
        if not flagged:
            return n, len(changed)
        rec = pic.mb_records()
        for (m, key) in flagged:
            if isinstance(key, tuple):
                at, size = RC.block_at(rec[m], 1 << (4 * key[1])) * 16, 64
            else:
                at, size = RC.block_at(rec[m], key) * 16, 16
            lv = pic.coefs[at:at + size].astype(np.int64)
            nz = np.flatnonzero(lv)
            half = np.where(lv < 0, -((-lv) >> 1), lv >> 1)
            if len(nz) and not half.any():
                half[nz[-1]] = 1 if lv[nz[-1]] > 0 else -1
            if size == 64:                                   # (each of the four entries keeps a level if it had one: the mask stays true)
                for j in range(4):
                    seg = lv[16 * j:16 * j + 16]
                    if seg.any() and not half[16 * j:16 * j + 16].any():
                        k = 16 * j + int(np.flatnonzero(seg)[-1])
                        half[k] = 1 if lv[k] > 0 else -1
            if np.array_equal(half, lv):                     # (nothing left to halve: weights above 16 at a high QP - the macroblock's QP steps down)
                rec["qp"][m] = max(int(rec["qp"][m]) - 6, 0)
            pic.coefs[at:at + size] = half.astype(np.int16)
            changed.add((m, key))
    raise AssertionError("make_conformant: still out of range after %d rounds" % max_rounds)


# ---- a picture ------------------------------------------------------------------------------------------------------------------
class _Residual(spec_recon._Residual):
    """IntraChecker's three hooks with the picture's lists"""
    census = None

    def _of(self, pic, r, x_mb, y_mb):
        m = y_mb * pic.desc.mb_w + x_mb
        if self.cache[0] != (id(pic), m):
            self.cache = ((id(pic), m), residual_of(pic, m, census=self.census)[0])
        return self.cache[1]


class IntraChecker(I8.IntraChecker):
    """i8x8_checker.IntraChecker whose Intra 8x8 macroblocks take their residual from here (that class asks its module's luma8x8_of and
    t8x8_checker's chroma_residual_of: both names stand for this module's functions while it runs)"""

    def _intra_mb(self, pic, m, F):
        keep = I8.luma8x8_of, T8.chroma_residual_of
        I8.luma8x8_of, T8.chroma_residual_of = luma8x8_of, chroma_residual_of
        try:
            return super()._intra_mb(pic, m, F)
        finally:
            I8.luma8x8_of, T8.chroma_residual_of = keep


class SpecRecon(I8.SpecRecon):
    """i8x8_checker.SpecRecon for pictures with scaling_lists: the list by macroblock kind and plane"""

    def __init__(self, mb_w, mb_h, slots):
        super().__init__(mb_w, mb_h, slots)
        self.scaling = Census()
        res = _Residual()
        res.census = self.scaling
        self.intra = IntraChecker(None, mb_w, mb_h, slots, residual=res, inter=self._inter, store=self.store)
        self.intra.census8 = self.census8
        self.scaled = 0                        # pictures with scaling_lists

    def _inter(self, pic):
        F = inter_checker.predict(pic, self.store, self.census)
        for m in np.flatnonzero(pic.mb_records()["mb_type"] > N.MB_IPCM):
            add_residual(pic, int(m), F, self.scaling)

    def reconstruct(self, pic):
        self.scaled += bool(int(pic.desc.scaling_lists))
        return super().reconstruct(pic)
