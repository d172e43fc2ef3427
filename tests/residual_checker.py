"""Checker for the residual (TEST INFRASTRUCTURE), written from the text of H.264 8.5 - not from oracle/cpu_recon.c
(oracle_dequant4x4 / oracle_idct4x4dc / oracle_add4x4_idct ... restate the reference's int16 functions), not from kernel_mc.h /
kernel_intra.h and not from the reference.  Python integers of unbounded size; nothing of the oracle is called or loaded.

Steps: the inverse zig-zag scan of frame macroblocks (8.5.6, table 8-13); the Intra16x16 luma DC transform and its scaling with
both branches qP >= 36 / qP < 36 (8.5.10); the chroma DC transform and scaling (8.5.11) at QP'c = table 8-15 of Clip3(0, 51, qp +
chroma_qp_offset) (8-bit video: QpBdOffset 0); the scaling of 4x4 blocks with flat matrices, LevelScale4x4 = 16 * normAdjust4x4, both
branches qP >= 24 / qP < 24 (8.5.12.1); the transform, rows then columns, (h + 32) >> 6 (8.5.12.2); picture construction with
Clip1 (8.5.14).  Blocks are found as include/p264hip.h lays them out: from coef_index [luma DC][chroma DC][blocks 0 .. 23 present
in coef_mask], sixteen levels each in scan order, AC-only blocks (Intra16x16 luma, chroma) hold their fifteen levels in [0 .. 14].

Range: 8.5.10 - 8.5.12 bound, for a conformant stream of 8-bit video, every d, e, f, g, h, dcY, dcC and every output (and
first-stage value) of the two DC transforms to -2^15 .. 2^15 - 1.  Outside that range H.264 defines no result (this project
follows the reference's int16 wrap there, SURVEY A-Q8, pinned by the oracle's tests); `block4x4`, `luma_dc` and `chroma_dc`
record every bounded value in a `Range` and `residual_of` REFUSES (OutOfRange) to produce samples for a macroblock with a value
outside.  `make_conformant(pic)` shrinks the levels of flagged blocks until the picture's census is clean."""
import numpy as np

from p264decoder_amd import _native as N

LO, HI = -(1 << 15), (1 << 15) - 1
# table 8-13, frame macroblocks: scan position -> (row i, column j) of c
ZIGZAG = [(0, 0), (0, 1), (1, 0), (2, 0), (1, 1), (0, 2), (0, 3), (1, 2), (2, 1), (3, 0), (3, 1), (2, 2), (1, 3), (2, 3), (3, 2), (3, 3)]
# table 8-15: qPI -> QPC
CHROMA_QP = list(range(30)) + [29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39]
# eq. 8-315: v[m] = normAdjust4x4 at positions (even, even), (odd, odd), the rest
V = [(10, 16, 13), (11, 18, 14), (13, 20, 16), (14, 23, 18), (16, 25, 20), (18, 29, 23)]
# 4x4 luma blocks in decoding order -> position in units of blocks (6.4.3)
BLK_X = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
BLK_Y = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]


class OutOfRange(ValueError):
    pass


class Range:
    """every value the standard bounds, as the steps produce them: n values seen, `bad` - the names of the out-of-range ones"""

    def __init__(self):
        self.n = 0
        self.bad = []

    def see(self, name, values):
        for v in values:
            self.n += 1
            if not LO <= v <= HI:
                self.bad.append(name)
        return values

    @property
    def ok(self):
        return not self.bad


def level_scale(m, i, j):
    """LevelScale4x4(m, i, j) with Flat_4x4_16 (eq. 8-313 .. 8-315)"""
    return 16 * (V[m][0] if i % 2 == 0 and j % 2 == 0 else V[m][1] if i % 2 == 1 and j % 2 == 1 else V[m][2])


def chroma_qp(qp, offset):
    return CHROMA_QP[min(max(qp + offset, 0), 51)]


def unscan(levels, ac_only=False):
    """8.5.6: sixteen levels (fifteen from scan position 1 when ac_only) -> c[i][j]"""
    c = [[0] * 4 for _ in range(4)]
    for k in range(15 if ac_only else 16):
        i, j = ZIGZAG[k + 1 if ac_only else k]
        c[i][j] = int(levels[k])
    return c


def luma_dc_transform(c, rng):
    """8.5.10, eq. 8-324: c[4][4] -> f[4][4]"""
    A = [[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]]
    t = [[sum(A[i][k] * c[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    f = [[sum(t[i][k] * A[k][j] for k in range(4)) for j in range(4)] for i in range(4)]
    rng.see("luma DC transform", [x for r in t for x in r])
    rng.see("luma DC f", [x for r in f for x in r])
    return f


def luma_dc(c, qp, rng):
    """8.5.10: c[4][4] -> dcY[4][4]"""
    f = luma_dc_transform(c, rng)
    ls = level_scale(qp % 6, 0, 0)
    if qp >= 36:
        dc = [[(x * ls) << (qp // 6 - 6) for x in r] for r in f]
    else:
        dc = [[(x * ls + (1 << (5 - qp // 6))) >> (6 - qp // 6) for x in r] for r in f]
    rng.see("dcY", [x for r in dc for x in r])
    return dc


def chroma_dc(c4, qpc, rng):
    """8.5.11: the four DC levels of one chroma plane (raster 2 x 2) -> dcC, raster"""
    c = [[int(c4[0]), int(c4[1])], [int(c4[2]), int(c4[3])]]
    A = [[1, 1], [1, -1]]
    t = [[sum(A[i][k] * c[k][j] for k in range(2)) for j in range(2)] for i in range(2)]
    f = [[sum(t[i][k] * A[k][j] for k in range(2)) for j in range(2)] for i in range(2)]
    rng.see("chroma DC f", [x for r in f for x in r])
    ls = level_scale(qpc % 6, 0, 0)
    dc = [((x * ls) << (qpc // 6)) >> 5 for r in f for x in r]
    rng.see("dcC", dc)
    return dc


def scale4x4(c, qp, rng, dc=None):
    """8.5.12.1: c[4][4] -> d[4][4]; dc: the already scaled d00 of an Intra16x16 luma or a chroma block"""
    m, s = qp % 6, qp // 6
    d = [[0] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            if dc is not None and i == 0 and j == 0:
                d[i][j] = dc
            elif qp >= 24:
                d[i][j] = (c[i][j] * level_scale(m, i, j)) << (s - 4)
            else:
                d[i][j] = (c[i][j] * level_scale(m, i, j) + (1 << (3 - s))) >> (4 - s)
    rng.see("d", [x for r in d for x in r])
    return d


def transform4x4(d, rng):
    """8.5.12.2: d[4][4] -> r[4][4]"""
    e = [[d[i][0] + d[i][2], d[i][0] - d[i][2], (d[i][1] >> 1) - d[i][3], d[i][1] + (d[i][3] >> 1)] for i in range(4)]
    f = [[e[i][0] + e[i][3], e[i][1] + e[i][2], e[i][1] - e[i][2], e[i][0] - e[i][3]] for i in range(4)]
    g = [[f[0][j] + f[2][j] for j in range(4)], [f[0][j] - f[2][j] for j in range(4)],
         [(f[1][j] >> 1) - f[3][j] for j in range(4)], [f[1][j] + (f[3][j] >> 1) for j in range(4)]]
    h = [[g[0][j] + g[3][j] for j in range(4)], [g[1][j] + g[2][j] for j in range(4)],
         [g[1][j] - g[2][j] for j in range(4)], [g[0][j] - g[3][j] for j in range(4)]]
    for name, a in (("e", e), ("f", f), ("g", g), ("h", h)):
        rng.see(name, [x for r in a for x in r])
    return [[(h[i][j] + 32) >> 6 for j in range(4)] for i in range(4)]


def block4x4(levels, qp, rng, ac_only=False, dc=None):
    """scan, scaling and transform of one 4x4 block: r[4][4]"""
    return transform4x4(scale4x4(unscan(levels, ac_only), qp, rng, dc), rng)


def construct(plane, x, y, r):
    """8.5.14: u = Clip1(pred + r), in place"""
    for i in range(4):
        for j in range(4):
            plane[y + i, x + j] = min(max(int(plane[y + i, x + j]) + r[i][j], 0), 255)


# ---- the layout of include/p264hip.h ----------------------------------------------------------------------------------------
def block_at(r, bit):
    """index, in blocks of sixteen levels, of the block `bit` (a coef_mask bit) of the macroblock with record r"""
    mask = int(r["coef_mask"])
    assert mask & bit, "block %#x is not present in mask %#x" % (bit, mask)
    if bit == N.COEF_LUMA_DC:
        k = 0
    elif bit == N.COEF_CHROMA_DC:
        k = 1 if mask & N.COEF_LUMA_DC else 0
    else:
        k = (1 if mask & N.COEF_LUMA_DC else 0) + (1 if mask & N.COEF_CHROMA_DC else 0) + bin(mask & (bit - 1) & 0xffffff).count("1")
    return int(r["coef_index"]) + k


def levels_of(pic, r, bit):
    at = block_at(r, bit) * 16
    return [int(v) for v in pic.coefs[at:at + 16]]


def residual_of(pic, m, refuse=True):
    """The residual of macroblock m (not I_PCM): ({(plane, x, y): r[4][4]} with x, y in samples inside the macroblock's area of
    the plane, the Range of everything bounded on the way, {coef_mask bit or COEF_*_DC: names out of range} per level block that
    fed an out-of-range value).  refuse: raise OutOfRange instead of returning samples the standard does not define."""
    r = pic.mb_records()[m]
    mask, qp, t = int(r["coef_mask"]), int(r["qp"]), int(r["mb_type"])
    assert t != N.MB_IPCM
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
    if t == N.MB_I16x16:
        dc = [[0] * 4 for _ in range(4)]
        if mask & N.COEF_LUMA_DC:
            dc = run([N.COEF_LUMA_DC], lambda g: luma_dc(unscan(levels_of(pic, r, N.COEF_LUMA_DC)), qp, g))
        for i in range(16):
            lv = levels_of(pic, r, 1 << i) if mask >> i & 1 else [0] * 16
            bits = ([1 << i] if mask >> i & 1 else []) + ([N.COEF_LUMA_DC] if mask & N.COEF_LUMA_DC else [])
            out[(0, BLK_X[i] * 4, BLK_Y[i] * 4)] = run(bits, lambda g: block4x4(lv, qp, g, True, dc[BLK_Y[i]][BLK_X[i]]))
    else:
        for i in range(16):
            if mask >> i & 1:
                out[(0, BLK_X[i] * 4, BLK_Y[i] * 4)] = run([1 << i], lambda g: block4x4(levels_of(pic, r, 1 << i), qp, g))
    if int(r["cbp"]) >> 4:
        qpc = chroma_qp(qp, int(pic.desc.chroma_qp_offset))
        for ch in range(2):
            has_dc = bool(mask & N.COEF_CHROMA_DC)
            dc = [0] * 4
            if has_dc:
                dc = run([N.COEF_CHROMA_DC], lambda g: chroma_dc(levels_of(pic, r, N.COEF_CHROMA_DC)[ch * 4:ch * 4 + 4], qpc, g))
            for i in range(4):
                b = 16 + ch * 4 + i
                lv = levels_of(pic, r, 1 << b) if mask >> b & 1 else [0] * 16
                bits = ([1 << b] if mask >> b & 1 else []) + ([N.COEF_CHROMA_DC] if has_dc else [])
                out[(1 + ch, (i & 1) * 4, (i >> 1) * 4)] = run(bits, lambda g: block4x4(lv, qpc, g, True, dc[i]))
    else:
        assert not mask & (0x00ff0000 | N.COEF_CHROMA_DC), "macroblock %d: chroma levels in the mask, none in cbp" % m
    if refuse and not total.ok:
        raise OutOfRange("macroblock %d: %s outside -2^15 .. 2^15 - 1: H.264 defines no result" % (m, sorted(set(total.bad))))
    return out, total, blame


def add_residual(pic, m, F, only=None):
    """8.5.14 for macroblock m on the planes F = [y, u, v], which hold its prediction.  only: a set of planes"""
    d = pic.desc
    x0, y0 = (m % d.mb_w) * 16, (m // d.mb_w) * 16
    for (plane, x, y), r in residual_of(pic, m)[0].items():
        if only is None or plane in only:
            construct(F[plane], (x0 >> (plane > 0)) + x, (y0 >> (plane > 0)) + y, r)


def census(pic):
    """(coded level blocks of the picture, {(macroblock, bit): names} of those that feed a value out of range)"""
    rec = pic.mb_records()
    n, flagged = 0, {}
    for m in range(pic.n_mb):
        if int(rec["mb_type"][m]) == N.MB_IPCM:
            continue
        mask = int(rec["coef_mask"][m])
        n += bin(mask & 0x03ffffff).count("1")
        if mask:
            for bit, names in residual_of(pic, m, refuse=False)[2].items():
                flagged[(m, bit)] = names
    return n, flagged


def make_conformant(pic, max_rounds=40):
    """Shrinks, in place in pic.coefs, the levels of every block that feeds an out-of-range value towards zero - halved, the last
    non-zero level of a block never below magnitude 1, so no block becomes all-zero and coef_mask stays true - until the census is
    clean.  Returns (coded blocks, blocks that were changed)."""
    changed = set()
    for _ in range(max_rounds):
        n, flagged = census(pic)
        if not flagged:
            return n, len(changed)
        rec = pic.mb_records()
        for (m, bit) in flagged:
            at = block_at(rec[m], bit) * 16
            lv = pic.coefs[at:at + 16].astype(np.int64)
            nz = np.flatnonzero(lv)
            half = np.where(lv < 0, -((-lv) >> 1), lv >> 1)
            if len(nz) and half[nz[-1]] == 0:
                half[nz[-1]] = 1 if lv[nz[-1]] > 0 else -1
            pic.coefs[at:at + 16] = half.astype(np.int16)
            changed.add((m, bit))
    raise AssertionError("make_conformant: still out of range after %d rounds" % max_rounds)
