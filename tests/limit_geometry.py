"""Pictures at the geometries where the kernels change path and at the limits p264hip_create accepts (TEST INFRASTRUCTURE), drawn at
the CPU->GPU seam from seeds with the means that exist (seam_fuzz.make_picture, inter_stim's Builder and vector_onto,
edge_geometry_stim.picture_set): nothing is data.

GEOMETRIES (mb_w, mb_h) and what each is on the list for - `switches()` restates the conditions from the headers' constants, read
out of the headers' text (`constants()`), and tests/test_limit_geometry_cpu.py holds every row to its claim:
    1 x 160    n_win == INTRA_MASKS: the last entries of m_intra / m_walk, use_free still on
    1 x 161    n_win 161: use_free off in P and B pictures; no left or right neighbour, 41 intra bands
    65 x 81    n_win 162 with two windows a row: the off path with window seams and top-right neighbours across them
    64 x 128   8192 macroblocks: the last geometry with `keep` (kernel_mc_sort.h), the largest the compact road takes (M = 8, no idle thread)
    64 x 129   8256: keep off with use_free still on (n_win 129); the compact road is refused
    33 x 32    1056: compact expansion with M = 2 and 496 idle threads
    3 x 512    row 511: 32 work-list bands without a knob, every entry of the progress arrays
    2047 x 2   column 2046: 32 intra windows a row, strip offsets up to 2046 * ystrip

Pictures.  `main_set(geometry)`: the Baseline / Main kinds, each named by what it makes the launch plan choose - an unweighted P
picture, an I picture (beside the P picture: dense k_intra, k_deblock_bs<false>), a B picture with implicit weights and two entries
per list, a P and a B picture with explicit weights.  The P and B pictures have an intra share of about 0.3: isolated intra
macroblocks (drawn, share 0.12) and forced clusters of three to five rows (`cluster_map`), placed so that on every geometry a cluster
spans a hand-over between intra bands (rows 4k + 3 and 4k + 4) and, on 65 x 81, the window seam (columns 63 and 64).
`high_set(geometry)`: the five High-profile pictures of edge_geometry_stim.picture_set - on HIGH_GEOMETRIES only: drawing them costs
19 ms a macroblock (the conformance census of every level block is Python), 150 s at 64 x 128, which no test of a few seconds can pay.
`fast_picture(geometry, kind)` (FAST_GEOMETRIES: every geometry above 161 macroblocks): a P picture with T8X8 records and Intra 8x8
macroblocks, a dense Intra 8x8 picture (Intra4x4, Intra16x16 and I_PCM between), a scaled B picture (JVT lists) and a scaled P picture with
explicit weights (random lists) - seam_fuzz.make_picture, then t8x8_stim's draw_block / insert and i8x8_stim's convert, the census of
every level block left to the golden file's generator (0.7 ms a macroblock to draw, 6 s at 64 x 129).
`scaled_picture(geometry)` / `cr_picture(geometry)`: an unweighted P picture with the JVT lists (SCALED_GEOMETRIES) / with a Cr QP offset
of its own (CR_GEOMETRIES), drawn by seam_fuzz.make_picture with levels tamed by rule (`tame`) instead of a census in the test.
`limit_vector_set(geometry)`: on 2047 x 2 macroblocks in columns 600 .. 1400 with x components from inter_stim.LIMITS_X, on 3 x 512
macroblocks in rows 150 .. 350 with y components from LIMITS_Y - a first group whose window lies wholly inside the reference
(unclamped key, strip offsets of megabytes), a second group of the same size whose window crosses a border of the short dimension by
one sample (clamped key); P and B, whole macroblocks and quadrants, every luma phase class; references are noise, so that a window
displaced by one strip shows.

Expectations.  Unweighted Baseline / Main pictures: the oracle (C), computed where they are needed.  Pictures with explicit weights:
tests/wp_checker.py, about 1.05 ms a macroblock here (33 x 32: 1.1 s; 64 x 129: 8.7 s) - computed in the test up to IN_TEST_MB
macroblocks, above that a SHA-256 per plane in tests/golden/limit_geometry.json.  High-profile pictures: scaling_checker.SpecRecon,
2 .. 2.7 ms a macroblock and picture (33 x 32: 2.1 .. 3.2 s a picture; 64 x 129: 16.8 s), with a Cr offset cr_offset_checker.TwoChains
over it (4.5 ms; 64 x 129: 36.9 s) - all of them in the golden file.  The file is written by
tests/golden/make_limit_geometry.py and holds seam_fuzz.picture_digest of every picture it covers."""
import collections
import ctypes as C
import functools
import hashlib
import json
import os
import re

import numpy as np

from p264decoder_amd import _native as N
from tests import edge_geometry_stim as E
from tests import inter_checker as IC
from tests import inter_stim as S
from tests import pcm_checker
from tests import seam_fuzz
from tests import worklist_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "p264decoder_amd", "csrc", "hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "limit_geometry.json")
Stim = collections.namedtuple("Stim", "name pic frames")

GEOMETRIES = ((1, 160), (1, 161), (65, 81), (64, 128), (64, 129), (33, 32), (3, 512), (2047, 2))
HIGH_GEOMETRIES = ((1, 160), (1, 161))
LIMIT_GEOMETRIES = ((2047, 2), (3, 512))
IDS = lambda g: "%dx%d" % g
SEED = 9300
SLOTS, DST = 3, 0                  # references in slots 1 and 2, every picture writes slot 0 (inter_stim.Builder's convention)
IN_TEST_MB = 1600                  # wp_checker in the test up to this many macroblocks (1.7 s), from the golden file above
WINDOW, BAND = E.WINDOW, E.BAND
MAIN = ("P", "I", "B implicit", "P weighted", "B weighted")
MAIN_ARGS = {"P": dict(n_ref=2), "I": dict(p_picture=False), "B implicit": dict(n_ref=2, n_ref_l1=2, b_picture=True, weighted=True),
             "P weighted": dict(n_ref=2, explicit_wp="legal"), "B weighted": dict(n_ref=2, n_ref_l1=2, b_picture=True, explicit_wp="legal")}


# ---- the headers' constants and the switches they set ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """{name: value} of the constants the switches are made of, out of the headers' text"""
    where = {"launch_shared.h": ("MC_SORT_THREADS", "MC_MAX_BANDS", "INTRA_ROW_WAVES", "MAX_PICS_PER_WG"), "kernel_mc_sort.h": ("MC_SORT_KEEP", "MCE_COL_BITS", "MCE_ROW_BITS"),
             "kernel_intra.h": ("INTRA_MASKS", "INTRA_BAND"), "kernel_expand.h": ("EXPAND_THREADS",), "wavefront_sync.h": ("MAX_MB_ROWS",),
             os.path.join(ROOT, "include", "p264hip.h"): ("P264HIP_COMPACT_MAX_MB", "P264HIP_COMPACT_MAGIC")}
    out = {}
    for path, names in where.items():
        text = open(path if os.path.isabs(path) else os.path.join(HIP, path)).read()
        for name in names:
            m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)u?\b" % name, text) or re.search(r"\b%s\s*=\s*(\d+)\b" % name, text)
            assert m, "%s: no %s" % (path, name)
            out[name] = int(m.group(1), 0)
    return out


def switches(geometry):
    """what the geometry sets in the kernels: keep (kernel_mc_sort.h, a P picture), n_win and use_free (kernel_intra.h, a P or B
    picture), M of k_expand_compact and whether the compact road takes the picture, the bands of the work lists (launch_plan.h) and of
    the intra kernels, the loop filter's bands at P264AMD_DEBLOCK_RB_LOG2 = 1"""
    c, (w, h) = constants(), geometry
    n_mb = w * h
    n_win = h * -(-w // WINDOW)
    lg = M.effective_band_log2(h)
    return {"n_mb": n_mb, "keep": n_mb <= c["MC_SORT_KEEP"] * c["MC_SORT_THREADS"], "n_win": n_win, "use_free": n_win <= c["INTRA_MASKS"] and n_mb < 65536,
            "M": -(-n_mb // c["EXPAND_THREADS"]), "idle": c["EXPAND_THREADS"] - -(-n_mb // -(-n_mb // c["EXPAND_THREADS"])), "compact": n_mb <= c["P264HIP_COMPACT_MAX_MB"],
            "mc_band_log2": lg, "mc_bands": M.n_bands(h, lg), "intra_bands": -(-h // c["INTRA_BAND"]), "deblock_bands_rb1": -(-h // 2),
            "last_col": w - 1, "last_row": h - 1}


def consistent_header(pic):
    """a compact block of zeros behind a header that is consistent for the picture, laid out as p264hip_pack_compact lays its
    sections out (no vector, no Intra4x4 entry, every level block narrow): what p264hip_compact_header_ok accepts for a picture of
    up to P264HIP_COMPACT_MAX_MB macroblocks - above it the limit is the only thing it can refuse.  Unweighted pictures without lists"""
    d = pic.desc
    assert not int(d.explicit_wp) and not int(d.scaling_lists)
    up16 = lambda v: (v + 15) & ~15
    n, nb = pic.n_mb, int(d.n_coef_blocks)
    h = N.CompactHdr()
    h.magic, h.n_mb, h.n_coef_blocks, h.n_lists = constants()["P264HIP_COMPACT_MAGIC"], n, nb, 2 if int(d.slice_type) == N.SLICE_B else 1
    h.off_rec = at = C.sizeof(N.CompactHdr)
    at = up16(at + n * 16)
    for l in range(h.n_lists):
        h.list[l].off_ref, at = at, up16(at + n * 4)
        h.list[l].off_shape, at = at, up16(at + (n + 3) // 4)
        h.list[l].off_vec, h.list[l].n_vec = at, 0
    h.off_i4flag, at = at, up16(at + (n + 7) // 8)
    h.off_i4, h.n_i4 = at, 0
    h.off_lvflag, at = at, up16(at + (nb + 7) // 8)
    h.off_levels, h.level_bytes = at, nb * 16
    at = up16(at + nb * 16) + 32
    if h.n_lists == 2:
        h.off_weights, at = at, at + 512
    h.bytes = at
    block = np.zeros(at, np.uint8)
    block[:C.sizeof(h)] = np.frombuffer(bytes(h), np.uint8)
    return block


# ---- intra clusters ----------------------------------------------------------------------------------------------------------------
def cluster_map(rng, mb_w, mb_h):
    """{macroblock: "i4" | "i16"}: clusters of three to five rows and up to six columns, about a sixth of the picture; the first
    starts at row 2 (it spans the hand-over of rows 3 and 4; row 0 of a picture of one or two rows), on a picture wider than a window at column 61 (it spans the seam)"""
    force, target = {}, max(mb_w * mb_h // 6, min(mb_w * mb_h, 5))
    first = True
    while len(force) < target:
        ch, cw = int(rng.integers(3, 6)), int(rng.integers(1, 7))
        y0 = (2 if mb_h > 2 else 0) if first else int(rng.integers(0, max(mb_h - ch, 0) + 1))
        x0 = (WINDOW - 3 if mb_w > WINDOW else 0) if first else int(rng.integers(0, max(mb_w - cw, 0) + 1))
        if first:
            ch, cw = 5, 6
        first = False
        for y in range(y0, min(y0 + ch, mb_h)):
            for x in range(x0, min(x0 + cw, mb_w)):
                force[y * mb_w + x] = "i4" if rng.random() < 0.5 else "i16"
    return force


@functools.lru_cache(maxsize=None)
def main_picture(geometry, kind, seed=SEED):
    """one kind's picture (drawn once per geometry and kind; the pictures are not to be changed)"""
    w, h = geometry
    rng = np.random.default_rng([seed, w, h, MAIN.index(kind)])
    wp = "weighted" in kind
    force = cluster_map(rng, w, h) if kind != "I" else None
    pic = seam_fuzz.make_picture(rng, w, h, slots=SLOTS, dst_slot=DST, level_style="small" if wp else "mixed", qp_mode="random", intra_share=0.12,
                                 slices=2, force=force, **MAIN_ARGS[kind])
    return Stim("%s %s" % (kind, IDS(geometry)), pic, S.frames_for(rng, w, h) if kind != "I" else {})


def main_set(geometry):
    """{kind: Stim}"""
    return {kind: main_picture(geometry, kind) for kind in MAIN}


@functools.lru_cache(maxsize=None)
def high_set(geometry):
    assert geometry in HIGH_GEOMETRIES
    return [Stim(st.name, st.pic, st.frames) for st in E.picture_set(*geometry)]


# ---- High-profile pictures that cost no census to draw -----------------------------------------------------------------------------
SCALED_GEOMETRIES = ((65, 81), (64, 129))                # the intra kernels' off path and the sort's second classification, scaled instances
CR_GEOMETRIES = ((64, 129), (3, 512), (2047, 2))


def tame(pic):
    """levels that stay inside the ranges of 8.5 at any QP without a census in the test (the generator of the golden file runs it and
    refuses the picture otherwise): a block keeps its first six levels in scan order, of magnitude at most 6; the blocks of
    macroblocks with a QP above 12 their first three, of magnitude at most 2 (QP up to 36) or 1"""
    rec = pic.mb_records()
    nb = int(pic.desc.n_coef_blocks)
    if not nb:
        return pic
    lv = pic.coefs[:nb * 16].reshape(nb, 16)
    owner = np.searchsorted(rec["coef_index"], np.arange(nb), side="right") - 1          # (coef_index never falls: the blocks lie in macroblock order)
    qp = rec["qp"][owner].astype(np.int64)
    top = np.where(qp > 36, 1, np.where(qp > 12, 2, 6))
    np.clip(lv, -top[:, None], top[:, None], out=lv)
    lv[:, 3:] *= (qp <= 12)[:, None].astype(np.int16)
    lv[:, 6:] = 0
    empty = ~lv.any(axis=1)
    lv[empty, 0] = 1
    return pic


def _high_p(geometry, what, seed):
    w, h = geometry
    rng = np.random.default_rng([seed, w, h])
    pic = seam_fuzz.make_picture(rng, w, h, slots=SLOTS, dst_slot=DST, level_style="small", qp_mode="random", intra_share=0.12, slices=2,
                                 force=cluster_map(rng, w, h), n_ref=2)
    return Stim("P %s %s" % (what, IDS(geometry)), tame(pic), S.frames_for(rng, w, h, kind="smooth"))


@functools.lru_cache(maxsize=None)
def scaled_picture(geometry, seed=SEED + 3):
    """an unweighted P picture with the JVT lists: alone it selects k_mc_sort_scaled_p, beside a B picture k_mc_sort_scaled"""
    from tests import scaling_checker as SC, scaling_stim as SS
    st = _high_p(geometry, "JVT lists", seed)
    SC.set_lists(st.pic, SS.jvt())
    return st


@functools.lru_cache(maxsize=None)
def cr_picture(geometry, seed=SEED + 4):
    """an unweighted P picture whose Cr has a QP offset of its own: k_deblock_bs_cr, k_deblock_cr"""
    st = _high_p(geometry, "Cr offset", seed)
    st.pic.desc.chroma_qp_offset, st.pic.desc.cr_qp_offset_delta = 5, -13
    return st


# ---- High-profile pictures with T8X8 records and Intra 8x8 macroblocks at every size ---------------------------------------------------
FAST_GEOMETRIES = ((65, 81), (64, 128), (64, 129), (33, 32), (3, 512), (2047, 2))
FAST = ("P T8X8 I8", "dense I8", "scaled B", "scaled weighted P")


class FastPlan(object):
    """i8x8_stim.Plan until every (mode, block, availability) case has been reached, then flags and modes by a table: Plan.take
    searches sixteen flag sets per macroblock, which a picture of thousands of Intra 8x8 macroblocks cannot pay"""

    def __init__(self, rng):
        from tests import i8x8_checker as I8, i8x8_stim as IS
        self.rng, self.plan, self.n_cases = rng, IS.Plan(rng), len(IS.all_cases())
        self.legal = {}
        for a in range(16):
            L, T, TR, TL = bool(a & N.AVAIL_LEFT), bool(a & N.AVAIL_TOP), bool(a & N.AVAIL_TOPRIGHT), bool(a & N.AVAIL_TOPLEFT)
            self.legal[a] = [I8.legal_modes(*I8.block_availability(k, L, T, TR, TL)[:3]) for k in range(4)]

    def take(self, allowed):
        if len(self.plan.seen) < self.n_cases:
            return self.plan.take(allowed)
        a = int(self.rng.integers(0, 16)) & allowed
        return a, [int(m[int(self.rng.integers(0, len(m)))]) for m in self.legal[a]]


def _owner(pic):
    rec, nb = pic.mb_records(), int(pic.desc.n_coef_blocks)
    return np.searchsorted(rec["coef_index"], np.arange(nb), side="right") - 1


def _to_t8x8(rng, pic, share):
    """t8x8_stim.drawn_picture's second half without its census: `share` of the inter macroblocks lose their 4x4 luma entries and get
    8x8 blocks drawn by t8x8_stim.draw_block (whose budget keeps them in range; t8x8_stim.insert checks each and halves)"""
    from tests import t8x8_stim as TS
    rec, nb = pic.mb_records(), int(pic.desc.n_coef_blocks)
    inter = rec["mb_type"] > N.MB_IPCM
    chosen = inter & (rng.random(pic.n_mb) < share)
    if nb:
        # the chosen macroblocks' luma entries leave the stream: within a macroblock the entries are chroma DC, luma, chroma AC
        owner = _owner(pic)
        first = rec["coef_index"][owner].astype(np.int64)
        has_dc = ((rec["coef_mask"][owner] & N.COEF_CHROMA_DC) != 0).astype(np.int64)
        n_l = np.array([bin(int(v) & 0xffff).count("1") for v in rec["coef_mask"]], np.int64)[owner]
        k = np.arange(nb) - first
        drop = chosen[owner] & (k >= has_dc) & (k < has_dc + n_l)
        keep = pic.coefs[:nb * 16].reshape(nb, 16)[~drop]
        counts = np.bincount(owner[~drop], minlength=pic.n_mb)
        rec["coef_index"] = np.concatenate([[0], np.cumsum(counts)[:-1]])
        rec["coef_mask"][chosen] &= ~np.uint32(0xffff)
        rec["cbp"][chosen] &= 0x30
        pic.desc.n_coef_blocks = len(keep)
        pic.coefs = np.concatenate([keep.reshape(-1), np.zeros(16, np.int16)]).astype(np.int16)
        pic.seal()
    blocks = {}
    for m in np.flatnonzero(chosen):
        skip = rec["mb_type"][m] == N.MB_P_SKIP
        cbp = 0 if skip else int(rng.integers(0, 16)) if rng.random() < 0.85 else 0
        blocks[int(m)] = {q: TS.draw_block(rng, int(rec["qp"][m])) for q in range(4) if cbp >> q & 1}
    return TS.insert(pic, blocks)


def _relax_for_lists(pic):
    """room for scaling weights of up to 64, two QP periods: every QP from 12 on goes down by 12; the levels of the other macroblocks
    are quartered (a coded block keeps a level)"""
    rec, nb = pic.mb_records(), int(pic.desc.n_coef_blocks)
    low = rec["qp"] < 12
    pcm = rec["mb_type"] == N.MB_IPCM
    rec["qp"][~low] -= 12
    if nb:
        lv = pic.coefs[:nb * 16].reshape(nb, 16)
        rows = (low & ~pcm)[_owner(pic)]
        q = np.sign(lv[rows]) * (np.abs(lv[rows]) >> 2)
        had = lv[rows] != 0
        lost = had.any(axis=1) & ~q.any(axis=1)
        firsts = had.argmax(axis=1)
        q[lost, firsts[lost]] = np.sign(lv[rows][lost, firsts[lost]])
        lv[rows] = q


@functools.lru_cache(maxsize=None)
def fast_picture(geometry, kind, seed=SEED + 5):
    """one of FAST at any geometry: seam_fuzz.make_picture, levels tamed by rule, T8X8 records by t8x8_stim's draw_block / insert, Intra 8x8
    macroblocks by i8x8_stim.convert (every fourth macroblock, the window seam, rows 3 and 4: edge_geometry_stim.flagged_of) - no census
    in the test; the generator of the golden file runs it and refuses a picture with a block out of range"""
    from tests import i8x8_stim as IS, pcm_fuzz, scaling_checker as SC, scaling_stim as SS
    w, h = geometry
    n = w * h
    rng = np.random.default_rng([seed, w, h, FAST.index(kind)])
    plan = FastPlan(rng)
    if kind == "dense I8":
        plain = [m for m in range(n) if ((m % w) + 3 * (m // w)) % 4 == 0]            # (i8x8_stim.dense_picture's pattern)
        kinds = {m: ("i4", "i16", "ipcm")[i % 3] for i, m in enumerate(plain)}
        force = {m: "i4" for m in range(n) if m not in kinds}
        force.update({m: k for m, k in kinds.items() if k != "ipcm"})
        pic = tame(seam_fuzz.make_picture(rng, w, h, p_picture=False, level_style="small", qp_mode="random", slices=1, slice_idcs=[0], force=force))
        chosen = np.zeros(n, bool)
        chosen[[m for m, k in kinds.items() if k == "ipcm"]] = True
        pcm_fuzz.to_ipcm(rng, pic, 0, samples="noise", chosen=chosen)
        IS.convert(pic, rng, {m for m in range(n) if m not in kinds}, plan)
        return Stim("%s %s" % (kind, IDS(geometry)), pic, {})
    flagged = E.flagged_of(w, h)
    kw = {"P T8X8 I8": {}, "scaled B": dict(b_picture=True, n_ref_l1=2), "scaled weighted P": dict(explicit_wp="legal")}[kind]
    pic = tame(seam_fuzz.make_picture(rng, w, h, slots=SLOTS, dst_slot=DST, level_style="small", qp_mode="random", mv_range=40, n_ref=2, intra_share=0.1,
                                      slices=1, slice_idcs=[0], force={m: "i4" for m in flagged}, **kw))
    _to_t8x8(rng, pic, 0.7)
    rec = pic.mb_records()
    IS.convert(pic, rng, set(flagged) | {int(m) for m in np.flatnonzero((rec["mb_type"] == N.MB_I4x4) & (rng.random(n) < 0.5))}, plan)
    if kind.startswith("scaled"):
        _relax_for_lists(pic)
        SC.set_lists(pic, SS.jvt() if kind == "scaled B" else SS.random_lists(seed + w))
    return Stim("%s %s" % (kind, IDS(geometry)), pic, S.frames_for(rng, w, h, kind="smooth"))


def fast_set(geometry):
    return {k: fast_picture(geometry, k) for k in FAST}


def assert_fast_covered(geometry, stims):
    """T8X8 records and Intra 8x8 macroblocks with levels, flat and scaled, in P, B and I pictures; Intra 8x8 on both sides of a band
    hand-over and, wider than a window, of the seam; the kinds' descriptors"""
    w, h = geometry
    d = {k: st.pic.desc for k, st in stims.items()}
    assert [int(d[k].slice_type) for k in FAST] == [N.SLICE_P, N.SLICE_I, N.SLICE_B, N.SLICE_P]
    assert [bool(int(d[k].scaling_lists)) for k in FAST] == [False, False, True, True] and [int(d[k].explicit_wp) for k in FAST] == [0, 0, 0, 1]
    for k, st in stims.items():
        rec = st.pic.mb_records()
        t = int(d[k].transform_8x8)
        coded = (rec["coef_mask"] & 0xffff) != 0
        i8 = (rec["mb_type"] == N.MB_I4x4) & ((rec["intra_modes"] & N.MB_I8X8) != 0)
        t8 = (rec["mb_type"] > N.MB_IPCM) & ((rec["intra_modes"] & N.MB_T8X8) != 0)
        assert t & N.T8X8_INTRA and (i8 & coded).sum() >= 8, (geometry, k)
        assert k == "dense I8" or (t & ~N.T8X8_INTRA and (t8 & coded).sum() >= 8), (geometry, k)
        a = i8.reshape(h, w)
        if h > BAND:
            assert (a[BAND - 1] & a[BAND]).any(), (geometry, k)
        if w > WINDOW:
            # both sides of the window seam: in every row, and the last column too (the dense picture: in a row, its pattern leaves every fourth plain)
            seam = a[:, WINDOW - 1] & a[:, WINDOW]
            assert seam.any() if k == "dense I8" else (seam.all() and a[:, w - 1].all()), (geometry, k)


def intra_of(pic):
    return (pic.mb_records()["mb_type"] <= N.MB_IPCM).reshape(pic.mb_h, pic.mb_w)


def assert_intra_covered(geometry, pic):
    """a P or B picture of main_set: the share, isolated macroblocks and clusters; with use_free all three roads of the sparse
    kernel; a cluster across a band hand-over and - wider than a window - across the window seam"""
    w, h = geometry
    a = intra_of(pic)
    share = a.mean()
    assert 0.2 <= share <= 0.4, "%s: intra share %.2f" % (geometry, share)
    p = np.pad(a, 1)
    alone = a & ~(p[1:-1, :-2] | p[1:-1, 2:] | p[:-2, 1:-1] | p[2:, 1:-1] | p[:-2, :-2] | p[:-2, 2:] | p[2:, :-2] | p[2:, 2:])
    assert alone.any(), "%s: no isolated intra macroblock" % (geometry,)
    assert h < 3 or (a[:-2] & a[1:-1] & a[2:]).any(), "%s: no cluster of three rows" % (geometry,)
    if switches(geometry)["use_free"]:
        roads = set(pcm_checker.sparse_roads(pic).tolist()) - {-1}
        assert roads == {0, 1, 2}, "%s: roads %s" % (geometry, roads)
    if h > BAND:
        over = [(y, x) for y in range(BAND - 1, h - 1, BAND) for x in range(w) if a[y, x] and a[y + 1, x]]
        assert over, "%s: no cluster across a band hand-over" % (geometry,)
        if w > WINDOW:
            assert any(a[y, WINDOW - 1] and a[y, WINDOW] and a[y + 1, WINDOW - 1] and a[y + 1, WINDOW] for y in range(BAND - 1, h - 1, BAND)), \
                "%s: no cluster across the window seam at a band hand-over" % (geometry,)


def assert_covered(geometry, stims):
    """main_set(geometry) holds what its kinds' names say"""
    d = {k: st.pic.desc for k, st in stims.items()}
    assert [int(d[k].slice_type) for k in MAIN] == [N.SLICE_P, N.SLICE_I, N.SLICE_B, N.SLICE_P, N.SLICE_B]
    assert [int(d[k].explicit_wp) for k in MAIN] == [0, 0, 0, 1, 1] and int(d["B implicit"].weighted_bipred) == 1
    assert all(int(d[k].n_ref) == 2 for k in MAIN if k != "I") and all(int(d[k].n_ref_l1) == 2 for k in MAIN if k.startswith("B"))
    for k in MAIN:
        if k != "I":
            assert_intra_covered(geometry, stims[k].pic)
    # the last row and the last column hold inter macroblocks: the top bits of a work-list entry's row and column fields
    inter = [~intra_of(stims[k].pic) for k in MAIN if k != "I"]
    assert any(a[-1].any() for a in inter) and any(a[:, -1].any() for a in inter), "%s: no inter macroblock in the last row / column" % (geometry,)
    for k in ("B implicit", "B weighted"):
        pic = stims[k].pic
        inter = np.repeat(pic.mb_records()["mb_type"] > N.MB_IPCM, 4)
        bi = inter & (pic.ref_idx >= 0) & (pic.ref_idx_l1 >= 0)
        assert bi.any() and (inter & (pic.ref_idx_l1 < 0)).any() and (inter & (pic.ref_idx < 0)).any(), "%s %s: not every list use" % (geometry, k)
        assert {0, 1} <= set(pic.ref_idx[bi].tolist()) and {0, 1} <= set(pic.ref_idx_l1[bi].tolist())


# ---- limit vectors inside the picture -----------------------------------------------------------------------------------------------
PHASES = [f for cls in IC.PHASE_CLASSES for f in S.FRACTIONS[cls][:1]]          # one luma phase of every class
LimitStim = collections.namedtuple("LimitStim", "name pic frames inside crossing")       # inside / crossing: [(macroblock, quadrant or None, list)]


def _limit_picture(geometry, b_picture, seed):
    """every macroblock inter with vector 0; in the span, every third macroblock carries a limit vector: by turns a whole macroblock
    and four quadrants, by turns with its window inside the reference and across the near border of the short dimension by one sample"""
    w, h = geometry
    wide = w > h
    rng = np.random.default_rng([seed, w, h, int(b_picture)])
    b = S.Builder(w, h, b_picture=b_picture, qp=27)
    pic = b.pic
    mv1 = pic.mv_l1.reshape(w * h, 16, 2)
    span = [m for m in range(w * h) if (600 <= m % w <= 1400 if wide else 150 <= m // w <= 350)][::3]
    inside, crossing = [], []
    for k, m in enumerate(span):
        x0, y0 = (m % w) * 16, (m // w) * 16
        cross, quads = bool(k & 1), bool(k & 2)
        lst = int(b_picture and bool(k & 4))                  # B pictures: list 0 and list 1 (bi-predicted: the other list keeps vector 0)
        if quads:
            pic.rec["mb_type"][m] = N.MB_B if b_picture else N.MB_P_8x8
        if b_picture:
            pic.ref_idx_l1[m * 4:m * 4 + 4] = int(rng.integers(0, 2))
            if k % 5 == 0:
                pic.ref_idx[m * 4:m * 4 + 4] = -1
                lst = 1
        pic.ref_idx[m * 4:m * 4 + 4] = np.where(pic.ref_idx[m * 4:m * 4 + 4] >= 0, int(rng.integers(0, 2)), -1)
        for q in (range(4) if quads else [None]):
            blocks = IC.quad_blocks(q) if quads else tuple(range(16))
            n, item = IC.LUMA_WINDOW["quad" if quads else "mb"]
            bx, by = x0 + (blocks[0] & 3) * 4, y0 + (blocks[0] >> 2) * 4
            frac = PHASES[int(rng.integers(0, len(PHASES)))]
            lim = int((S.LIMITS_X if wide else S.LIMITS_Y)[int(rng.integers(0, 4))])
            size = (h if wide else w) * 16                     # the short dimension: the window's place in it is chosen
            lo = (-1 if rng.random() < 0.5 else size - n + 1) if cross else int(rng.integers(0, size - n + 1))
            if wide:
                vx, vy = lim, S.vector_onto(0, lo, bx, by, frac, False, rng)[1]
            else:
                vx, vy = S.vector_onto(lo, 0, bx, by, frac, False, rng)[0], lim
            (mv1 if lst else b.mv)[m, list(blocks)] = (vx, vy)
            (crossing if cross else inside).append((m, q, lst))
        if k % 3 == 0:
            S._code_item(rng, b, m, list(range(16)))
    st = S.stim("limit vectors %s %s" % ("B" if b_picture else "P", IDS(geometry)), b.finish(), S.frames_for(rng, w, h))
    return LimitStim(st.name, st.pic, st.frames, inside, crossing)


@functools.lru_cache(maxsize=None)
def limit_vector_set(geometry, seed=SEED + 1):
    assert geometry in LIMIT_GEOMETRIES
    return [_limit_picture(geometry, False, seed), _limit_picture(geometry, True, seed)]


def weighted_twin(st, seed=SEED + 2):
    """the same picture with a table of explicit weights (a copy: the arrays are shared, the descriptor is not)"""
    import ctypes as C
    twin = seam_fuzz.SeamPicture(st.pic.mb_w, st.pic.mb_h)
    C.memmove(C.byref(twin.desc), C.byref(st.pic.desc), C.sizeof(N.Picture))
    for name in ("rec", "mv", "ref_idx", "i4modes", "coefs", "mv_l1", "ref_idx_l1"):
        setattr(twin, name, getattr(st.pic, name))
    twin.seal()
    seam_fuzz.draw_wp_table(np.random.default_rng([seed, st.pic.mb_w, st.pic.mb_h, int(st.pic.desc.slice_type)]), twin, "legal")
    return Stim(st.name + " weighted", twin, st.frames)


def assert_limit_covered(st):
    """the first group is filed under unclamped keys, the second under clamped ones (worklist_model), the vectors are limit vectors,
    and both groups have whole macroblocks and quadrants and every phase class"""
    pic = st.pic
    wide = pic.mb_w > pic.mb_h
    lims = set(S.LIMITS_X if wide else S.LIMITS_Y)
    assert len(st.inside) >= 24 and abs(len(st.inside) - len(st.crossing)) <= 4, (len(st.inside), len(st.crossing))
    seen = {False: set(), True: set()}
    for group, clamp in ((st.inside, False), (st.crossing, True)):
        for m, q, lst in group:
            assert (600 <= m % pic.mb_w <= 1400) if wide else (150 <= m // pic.mb_w <= 350)
            blocks = IC.quad_blocks(q) if q is not None else tuple(range(16))
            a = pic.mv_l1 if lst else pic.mv
            vec = IC._vec(a, m, blocks[0])
            assert vec[0 if wide else 1] in lims, vec
            kind = "mb" if q is None else "quad"
            assert M._inside(pic, m, kind, blocks, vec, False) == (not clamp), "%s: macroblock %d, vector %s" % (st.name, m, vec)
            filed = M.macroblock(pic, m)[0]
            ps = int(bool(lst) and int(pic.ref_idx[m * 4]) >= 0)             # (a bi-predicted macroblock's list-1 vector: the second pass)
            keys = [key for p, l, key, n in filed if l == ("YM" if q is None else "YQ") and p == ps]
            assert keys and all(bool(key & M.MCY_CLAMP) == clamp for key in keys), (m, q, lst, filed)
            seen[clamp].add((kind, IC.phase_class(vec[0] & 3, vec[1] & 3)))
    for clamp in (False, True):
        assert {k for k, _ in seen[clamp]} == {"mb", "quad"} and {p for _, p in seen[clamp]} == set(IC.PHASE_CLASSES), (clamp, seen[clamp])


# ---- the golden file ---------------------------------------------------------------------------------------------------------------
def plane_hashes(planes):
    return [hashlib.sha256(np.ascontiguousarray(p).tobytes()).hexdigest() for p in planes]


def golden_pictures():
    """[(key, Stim, checker name)] of every picture whose expectation the golden file holds"""
    out = []
    for g in GEOMETRIES:
        if g[0] * g[1] > IN_TEST_MB:
            out += [("%s/%s" % (IDS(g), k), main_picture(g, k), "wp_checker") for k in ("P weighted", "B weighted")]
    for g in LIMIT_GEOMETRIES:
        if g[0] * g[1] > IN_TEST_MB:
            out += [("%s/%s" % (IDS(g), st.name), weighted_twin(st), "wp_checker") for st in limit_vector_set(g)]
    out += [("%s/scaled P" % IDS(g), scaled_picture(g), "SpecRecon") for g in SCALED_GEOMETRIES]
    out += [("%s/Cr P" % IDS(g), cr_picture(g), "TwoChains") for g in CR_GEOMETRIES]
    out += [("%s/%s" % (IDS(g), k), fast_picture(g, k), "SpecRecon") for g in FAST_GEOMETRIES for k in FAST]
    for g in HIGH_GEOMETRIES:
        out += [("%s/high/%d %s" % (IDS(g), i, st.name), st, "SpecRecon") for i, st in enumerate(high_set(g))]
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))["pictures"]


def expected(oracle, st, key=None):
    """[y, u, v] of a Baseline / Main stimulus by the oracle (explicit weights: wp_checker), or - key - the golden file's hashes"""
    from tests import wp_checker
    if key is not None:
        entry = golden()[key]
        assert entry["digest"] == seam_fuzz.picture_digest(st.pic), "%s: the drawn picture is not the golden file's" % key
        return entry["planes"]
    chk = wp_checker.WeightedChecker(oracle, st.pic.mb_w, st.pic.mb_h, SLOTS)
    for slot, f in st.frames.items():
        for dst, src in zip(chk.store[slot], f):
            dst[:] = src
    return [p.copy() for p in chk.reconstruct(st.pic)]


def main_key(geometry, kind):
    """the golden key of a main_set picture, None where the test computes the expectation"""
    return "%s/%s" % (IDS(geometry), kind) if "weighted" in kind and geometry[0] * geometry[1] > IN_TEST_MB else None
