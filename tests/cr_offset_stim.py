"""Pictures whose Cr has a QP offset of its own (TEST INFRASTRUCTURE), built at the CPU->GPU seam from seeds: the pictures of the
stimulus modules that exist (tests/t8x8_stim.py: drawn P and B pictures with sparse intra macroblocks, with and without P264_MB_T8X8;
tests/i8x8_stim.py: dense I pictures of Intra16x16, Intra4x4, Intra 8x8 and I_PCM macroblocks, P pictures with Intra 8x8 among inter
macroblocks; tests/scaling_stim.py's lists) with a cr_qp_offset_delta, per-macroblock `flags` deltas on the filter offsets, and
brought into the ranges of 8.5 under BOTH chroma offsets (tests/cr_offset_checker.py: make_conformant).

`directed_set()`: I, P with sparse intra and B pictures at 1 x 1, 2 x 5, 9 x 1, 11 x 9 and 70 x 3 (more columns than a wavefront has
lanes), every pair of chroma_qp_offset -12 / 0 / 12 and delta -24 / -13 / -1 / +1 / +7 / +24; then one picture each with scaling
lists (Cb and Cr lists that differ), P264_MB_T8X8, P264_MB_I8X8, explicit weights, I_PCM macroblocks next to coded ones, and one
with deblock = 0.  `flat_set()`: pictures of the sizes above with delta 0 (plain and with lists) for mixed batches."""
import collections

import numpy as np

from tests import cr_offset_checker as CR
from tests import i8x8_stim as IS
from tests import pcm_fuzz
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import t8x8_stim as TS

Stim = collections.namedtuple("Stim", "name pic frames")
OFFSETS = (-12, 0, 12)
DELTAS = (-24, -13, -1, 1, 7, 24)
PAIRS = [(o, d) for d in DELTAS for o in OFFSETS]
SLOTS = 3
BATCH_W, BATCH_H = 6, 5                      # the pictures that meet in mixed batches


def flag_deltas(rng, pic, spread=6):
    """per-macroblock deltas on the picture's filter offsets (p264hip_mb_t.flags), a third of the macroblocks"""
    rec = pic.mb_records()
    for m in range(pic.n_mb):
        if rng.random() < 0.34:
            a, b = (int(v) for v in rng.integers(-spread, spread + 1, size=2))
            rec["flags"][m] = (a & 0xff) | ((b & 0xff) << 8)


def finish(st, rng, cqo, delta, name=None, flags=True):
    pic = st.pic
    pic.desc.chroma_qp_offset, pic.desc.cr_qp_offset_delta = cqo, delta
    if flags and int(pic.desc.deblock):
        flag_deltas(rng, pic)
        if not int(pic.desc.alpha_c0_offset) and not int(pic.desc.beta_offset):
            pic.desc.alpha_c0_offset, pic.desc.beta_offset = 3, -2
    if int(pic.desc.n_coef_blocks):
        CR.make_conformant(pic, SC.make_conformant)
    return Stim("%s cqo %d delta %d" % (name or st.name, cqo, delta), pic, st.frames)


def i_picture(rng, w, h, deblock=True):
    return IS.dense_picture(rng, IS.Plan(rng), "I %dx%d" % (w, h), deblock=deblock, mb_w=w, mb_h=h)


def p_picture(rng, w, h, share=0.0, **kw):
    kw.setdefault("intra_share", 0.15)
    kw.setdefault("slices", 1 if w * h < 4 else 2)
    return TS.drawn_picture(rng, "P %dx%d" % (w, h), w, h, share=share, **kw)


def b_picture(rng, w, h, share=0.0, **kw):
    kw.setdefault("intra_share", 0.1)
    kw.setdefault("slices", 1)
    return TS.drawn_picture(rng, "B %dx%d" % (w, h), w, h, share=share, b_picture=True, **kw)


def with_ipcm(rng, st, share=0.2):
    pcm_fuzz.to_ipcm(rng, st.pic, share, samples="noise")
    return st


def directed_set(seed=9100):
    rng = np.random.default_rng(seed)
    pairs = iter(PAIRS * 2)
    out = []
    for w, h in ((1, 1), (2, 5), (9, 1), (11, 9), (70, 3)):
        kinds = (i_picture, p_picture, b_picture) if w * h < 200 else (p_picture,)
        for make in kinds:
            out.append(finish(make(rng, w, h), rng, *next(pairs)))
    w, h = BATCH_W, BATCH_H
    # scaling lists whose Cb and Cr lists differ (random_lists draws every list on its own), in a P and in an I picture
    for make, lists in ((p_picture, SS.random_lists(31)), (i_picture, SS.ramp_lists())):
        st = make(rng, w, h)
        SC.set_lists(st.pic, lists)
        assert lists[1] != lists[2] and lists[4] != lists[5]
        out.append(finish(st, rng, *next(pairs), name="lists " + st.name))
    out.append(finish(p_picture(rng, w, h, share=0.7), rng, *next(pairs), name="T8X8 P"))
    out.append(finish(b_picture(rng, w, h, share=0.7), rng, *next(pairs), name="T8X8 B"))
    out.append(finish(IS.inter_picture(rng, IS.Plan(rng), "I8X8 P", IS.CLUSTER, 0.5, slices=1, slice_idcs=[0]), rng, *next(pairs)))
    out.append(finish(p_picture(rng, w, h, explicit_wp="legal"), rng, *next(pairs), name="weighted P"))
    out.append(finish(b_picture(rng, w, h, explicit_wp="legal"), rng, *next(pairs), name="weighted B"))
    out.append(finish(with_ipcm(rng, p_picture(rng, w, h, slice_idcs=[0, 0])), rng, *next(pairs), name="I_PCM P"))
    out.append(finish(with_ipcm(rng, b_picture(rng, w, h, slice_idcs=[0])), rng, *next(pairs), name="I_PCM B"))
    out.append(finish(p_picture(rng, w, h, slices=1, slice_idcs=[1]), rng, *next(pairs), name="unfiltered P"))
    assert {(int(s.pic.desc.chroma_qp_offset), int(s.pic.desc.cr_qp_offset_delta)) for s in out} == set(PAIRS)
    return out


def flat_set(seed=9101):
    """delta 0: a plain P picture, a P picture with lists, a B picture and an I picture of BATCH_W x BATCH_H"""
    rng = np.random.default_rng(seed)
    w, h = BATCH_W, BATCH_H
    out = [finish(p_picture(rng, w, h), rng, 5, 0, name="flat P")]
    st = p_picture(rng, w, h)
    SC.set_lists(st.pic, SS.jvt())
    out.append(finish(st, rng, -3, 0, name="lists P"))
    out.append(finish(b_picture(rng, w, h), rng, 0, 0, name="flat B"))
    out.append(finish(i_picture(rng, w, h), rng, 2, 0, name="flat I"))
    return out


def batch_set(seed=9102):
    """BATCH_W x BATCH_H pictures with a delta for the mixed batches: P, B, I, P with lists"""
    rng = np.random.default_rng(seed)
    w, h = BATCH_W, BATCH_H
    out = [finish(p_picture(rng, w, h), rng, 0, -13, name="cr P"), finish(b_picture(rng, w, h), rng, 12, -24, name="cr B"),
           finish(i_picture(rng, w, h), rng, -12, 24, name="cr I")]
    st = p_picture(rng, w, h, share=0.5)
    SC.set_lists(st.pic, SS.random_lists(32))
    out.append(finish(st, rng, 3, 7, name="cr lists T8X8 P"))
    return out


# ---- whole streams (synth264 --cqo2: the PPS extension's second_chroma_qp_index_offset) ------------------------------------------
# --qp / --qp-delta / --maxlevel: chosen so that every level block stays inside the ranges of 8.5 under both offsets and the QP chain of a
# picture of 99 macroblocks never leaves 0 .. 51 (the stream tests assert a clean census on every picture)
STREAM_COMMON = "--mbw 11 --mbh 9 --frames 7 --refs 2 --t8x8 50 --qp 20 --qp-delta 1 --coded 35 --maxlevel 2"
STREAMS = {"cavlc p": STREAM_COMMON + " --seed 91", "cabac b": STREAM_COMMON + " --bframes 2 --d8inf --cabac --seed 92"}
CQO, CQO2 = 3, -7


def stream_args(which, cqo=CQO, cqo2=CQO2):
    """the writer's arguments; cqo2 = None: the same stream without --cqo2"""
    return STREAMS[which] + " --cqo %d" % cqo + ("" if cqo2 is None else " --cqo2 %d" % cqo2)
