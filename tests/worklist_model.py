"""The work lists of the motion-compensation stage as a model (TEST INFRASTRUCTURE): which (band, key) of which list every inter
macroblock is filed under, restated in plain Python from the list rules documented in
p264decoder_amd/csrc/hip/kernel_mc_sort.h ("work lists", struct McMb) on top of inter_checker.classify (item kinds, roads) and inter_checker.phase_class.  Nothing compiled from the
kernels is imported; the lists themselves are never read back from the device - the model only PROVES what a stimulus asks of the
sort (tests/test_worklist_cpu.py), the pictures are what the GPU test observes.

Keys (kernel_mc_sort.h): luma = phase class | MCY_CLAMP | MCY_RESID, chroma = MCC_CLAMP | MCC_RESID | MCC_BI.  The rules:
* a macroblock with one vector, one reference (and, B pictures, one role) is one item of YM and one of CM; else its quadrants are
  items of YQ and its four chroma entries - always together, one key for all four - items of CQ;
* the window of an item (inter_checker.item_window) inside the picture or not gives CLAMP; a quadrant whose 4x4 blocks differ is
  PC_GEN | MCY_CLAMP and makes the macroblock's chroma key clamped;
* RESID: the item has coded luma blocks / the macroblock has any chroma level;
* explicit weights: every quadrant PC_GEN (no clamp), chroma MCC_BI, first pass only;
* a two-list macroblock of a B picture with vectors differing inside a quadrant of a list it uses: the same generic class;
* other two-list macroblocks: first pass, every quadrant with its list-0 vector (list 1 where it has no list 0), Z - no RESID - on
  bi-predicted ones (a split macroblock's chroma key keeps RESID: the Z rides in the entries); second pass, the bi-predicted
  quadrants with their list-1 vector and the residual, "not mine" quadrants without a luma entry, and - unless the macroblock is
  one item there - all four chroma entries, the carried ones (MCE_KEEP) tested with vector 0.
Pictures with the 8x8 transform or scaling lists file their residuals elsewhere and are not modelled."""
import collections

import numpy as np

from p264decoder_amd import _native as N
from tests import inter_checker as IC

# ---- typed from p264decoder_amd/csrc/hip/launch_shared.h and kernel_mc_sort.h; test_worklist_cpu.py holds them to the header ----
MCY_KEYS, MCC_KEYS, MC_MAX_BANDS = 32, 8, 32
LISTS = ("YM", "YQ", "CM", "CQ")                            # ML_YM .. ML_CQ in this order
CHUNK = {"YM": 4, "YQ": 16, "CM": 8, "CQ": 32}              # mc_chunk_items
LIST_KEYS = {"YM": MCY_KEYS, "YQ": MCY_KEYS, "CM": MCC_KEYS, "CQ": MCC_KEYS}
MC_KEY_SLOTS = 2 * MC_MAX_BANDS * MCY_KEYS + 2 * MC_MAX_BANDS * MCC_KEYS
PC = {name: i for i, name in enumerate(IC.PHASE_CLASSES)}   # copy 0 .. cv 6
PC_GEN = 7
MCY_CLAMP, MCY_RESID = 8, 16
MCC_CLAMP, MCC_RESID, MCC_BI = 1, 2, 4
DEFAULT_BAND_LOG2, MAX_BAND_KNOB = 4, 9                     # launch_plan.h: launch_device

# ---- the keys a picture kind can reach, per pass and list (the table DESIGN.md quotes) ----
_Y28 = frozenset(pc | c | r for pc in range(7) for c in (0, MCY_CLAMP) for r in (0, MCY_RESID))          # a uniform vector: never PC_GEN
_Y30 = _Y28 | {PC_GEN | MCY_CLAMP, PC_GEN | MCY_CLAMP | MCY_RESID}                                      # + vectors differing inside a quadrant
_Y32 = _Y30 | {PC_GEN, PC_GEN | MCY_RESID}                                                              # + the generic two-list class
_C4 = frozenset(range(4))
_C6 = _C4 | {MCC_BI, MCC_BI | MCC_RESID}                                                                # (MCC_BI never with MCC_CLAMP)
REACHABLE = {
    "P": {(0, "YM"): _Y28, (0, "YQ"): _Y30, (0, "CM"): _C4, (0, "CQ"): _C4},
    "B": {(0, "YM"): _Y28, (0, "YQ"): _Y32, (0, "CM"): _C4, (0, "CQ"): _C6,
          (1, "YM"): _Y28, (1, "YQ"): _Y28, (1, "CM"): _C4, (1, "CQ"): _C4},
    "WP": {(0, "YM"): frozenset(), (0, "YQ"): frozenset({PC_GEN, PC_GEN | MCY_RESID}), (0, "CM"): frozenset(),
           (0, "CQ"): frozenset({MCC_BI, MCC_BI | MCC_RESID})},
}


def kind_of(pic):
    d = pic.desc
    assert d.slice_type in (N.SLICE_P, N.SLICE_B)
    if d.explicit_wp:
        assert d.slice_type == N.SLICE_P, "explicit weights in B pictures: both passes' tables are not stated here"
        return "WP"
    return "B" if d.slice_type == N.SLICE_B else "P"


def effective_band_log2(mb_h, knob=None):
    """launch_plan.h, launch_device: P264AMD_MC_BAND_LOG2 in 0 .. 9 is taken, anything else is 16 rows; then the band doubles until
    the picture has at most MC_MAX_BANDS of them"""
    lg = knob if knob is not None and 0 <= knob <= MAX_BAND_KNOB else DEFAULT_BAND_LOG2
    while (mb_h + (1 << lg) - 1) >> lg > MC_MAX_BANDS:
        lg += 1
    return lg


def n_bands(mb_h, band_log2):
    return (mb_h + (1 << band_log2) - 1) >> band_log2


def needed_chunks(counter, per):
    return sum(-(-n // per) for n in counter.values())


def _inside(pic, m, kind, blocks, vec, chroma):
    x, y, n = IC.item_window(pic, m, kind, blocks, vec, chroma)
    W, H = pic.mb_w * 16 >> chroma, pic.mb_h * 16 >> chroma
    return IC.inside(IC.side(x, n, W) + IC.side(y, n, H))


def _luma_key(pic, m, kind, blocks, vec, coded):
    pc = PC[IC.phase_class(vec[0] & 3, vec[1] & 3)]
    return pc | (0 if _inside(pic, m, kind, blocks, vec, False) else MCY_CLAMP) | (MCY_RESID if coded else 0)


def macroblock(pic, m):
    """what inter macroblock m files: [(pass, list, key, items)] and the number of its carried (MCE_KEEP) chroma entries"""
    d = pic.desc
    assert not int(d.transform_8x8) and not int(d.scaling_lists), "not modelled"
    items, road = IC.classify(pic, m)
    mask = int(pic.mb_records()["coef_mask"][m])
    cc = bool(mask & (0x00ff0000 | N.COEF_CHROMA_DC))
    qcoded = [any(mask >> IC.DECODE_INDEX[bb] & 1 for bb in IC.quad_blocks(q)) for q in range(4)]
    out = []
    if road in ("wp", "generic"):
        for q in range(4):
            out.append((0, "YQ", PC_GEN | (MCY_RESID if qcoded[q] else 0), 1))
        out.append((0, "CQ", MCC_BI | (MCC_RESID if cc else 0), 4))
        return out, 0
    L = [IC.quadrant_lists(pic, m, q) for q in range(4)]
    two = road not in ("p", "list0 only")
    bi = [two and u0 and u1 for (u0, u1, e0, e1) in L]
    keep = 0
    for ps in (0, 1):
        if ps and not any(bi):
            break
        # the quadrant's item of this pass: (kind, blocks, vector) by classify, None = "not mine"
        ent = []
        for q in range(4):
            b0 = IC.quad_blocks(q)[0]
            l = 1 if ps else (0 if L[q][0] else 1)
            ent.append(items[(l, b0)] if (bi[q] if ps else True) else None)
        z = [bool(bi[q]) and not ps for q in range(4)]                      # first pass of a bi-predicted quadrant: no residual yet
        if ent[0] is not None and ent[0][0] == "mb":
            kind, blocks, vec = ent[0]
            out.append((ps, "YM", _luma_key(pic, m, kind, blocks, vec, any(qcoded) and not z[0]), 1))
            out.append((ps, "CM", (0 if _inside(pic, m, kind, blocks, vec, True) else MCC_CLAMP) | (MCC_RESID if cc and not z[0] else 0), 1))
            continue
        c_inside = True
        for q in range(4):
            qb = IC.quad_blocks(q)
            if ent[q] is None:
                keep += 1
                c_inside &= _inside(pic, m, "quad", qb, (0, 0), True)
                continue
            kind, blocks, vec = ent[q]
            if kind == "lane":
                out.append((ps, "YQ", PC_GEN | MCY_CLAMP | (MCY_RESID if qcoded[q] and not z[q] else 0), 1))
                c_inside = False
            else:
                assert kind == "quad" and blocks == qb
                out.append((ps, "YQ", _luma_key(pic, m, kind, blocks, vec, qcoded[q] and not z[q]), 1))
                c_inside &= _inside(pic, m, kind, blocks, vec, True)
        out.append((ps, "CQ", (0 if c_inside else MCC_CLAMP) | (MCC_RESID if cc else 0), 4))
    return out, keep


def lists(pic, band_log2):
    """{(pass, list): Counter of (band, key) -> items}: pass 0, and 1 for B pictures; list one of LISTS"""
    d = pic.desc
    passes = (0, 1) if d.slice_type == N.SLICE_B else (0,)
    out = {(ps, l): collections.Counter() for ps in passes for l in LISTS}
    rec = pic.mb_records()
    for m in np.flatnonzero(rec["mb_type"] > N.MB_IPCM):
        m = int(m)
        band = (m // pic.mb_w) >> band_log2
        for ps, l, key, n in macroblock(pic, m)[0]:
            assert 0 <= key < LIST_KEYS[l]
            out[(ps, l)][(band, key)] += n
    return out


def keep_entries(pic):
    """carried (MCE_KEEP) chroma entries of the second pass"""
    rec = pic.mb_records()
    return sum(macroblock(pic, int(m))[1] for m in np.flatnonzero(rec["mb_type"] > N.MB_IPCM))


def populated(counter, band=None):
    """the keys with items, of one band or of the whole picture"""
    return {k for (b, k), n in counter.items() if n and (band is None or b == band)}
