"""tests/spec_recon.py - a whole picture from the text of H.264 alone - against the oracle (CPU), byte for byte: on every directed
picture of tests/inter_stim.py, on the pictures of test_gpu_seam_fuzz.CONFIGS at the seeds that file uses, made conformant
(residual_checker.make_conformant: outside the range H.264 bounds there is no result to compare - the oracle's int16 wrap there is
pinned to the reference by tests/test_oracle_kat.py and to the kernels by the seam fuzz itself), and on the explicit-weight and
I_PCM fuzz configurations (the oracle's side composed by tests/pcm_checker.py, as their GPU files do).  Where the two differ the
finding is in the oracle or the stimulus, never in the checker."""
import os

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import inter_stim as S
from tests import pcm_checker, pcm_fuzz, residual_checker, seam_fuzz, spec_recon
from tests import ipcm_seam_stim as ipcm_cfg
from tests import wp_seam_stim as wp_cfg
from tests.stream_args import SEAM_CONFIGS

SETS = S.SETS


def first_difference(got, want, pic):
    for plane, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            s = 16 if plane == 0 else 8
            m = (ys[0] // s) * pic.mb_w + xs[0] // s
            r = pic.mb_records()[m]
            return "plane %d: %d samples differ, first (y=%d, x=%d) macroblock %d type %d qp %d mask %#x: standard %d oracle %d" % (
                plane, len(ys), ys[0], xs[0], m, r["mb_type"], r["qp"], r["coef_mask"], a[ys[0], xs[0]], b[ys[0], xs[0]])
    return None


def compare_stims(oracle, stims):
    """every picture through spec_recon and through the oracle; returns the name and first difference of the pictures that differ"""
    bad = []
    for st in stims:
        pic = st.pic
        ref = pcm_checker.PcmChecker(oracle, pic.mb_w, pic.mb_h, 3)
        spec = spec_recon.SpecRecon(pic.mb_w, pic.mb_h, 3)
        for slot, f in st.frames.items():
            spec.store.write(slot, f)
            for dst, src in zip(ref.store[slot], f):
                dst[:] = src
        d = first_difference(spec.reconstruct(pic), ref.reconstruct(pic), pic)
        if d:
            bad.append("%s: %s" % (st.name, d))
    return bad


@pytest.mark.parametrize("which", SETS)
def test_directed_pictures_equal_the_oracle(oracle, which):
    bad = compare_stims(oracle, getattr(S, which)())
    assert not bad, "%d pictures differ: %s" % (len(bad), bad[:3])


def run_chain(oracle, mb_w, mb_h, slots, frames, pictures, what):
    ref = pcm_checker.PcmChecker(oracle, mb_w, mb_h, slots)
    spec = spec_recon.SpecRecon(mb_w, mb_h, slots)
    for s, f in enumerate(frames):
        spec.store.write(s, f)
        for dst, src in zip(ref.store[s], f):
            dst[:] = src
    coded = changed = 0
    for i, pic in enumerate(pictures):
        n, c = residual_checker.make_conformant(pic)
        coded += n
        changed += c
        d = first_difference(spec.reconstruct(pic), ref.reconstruct(pic), pic)
        assert d is None, "%s picture %d: %s" % (what, i, d)
    return coded, changed, spec.census


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", SEAM_CONFIGS, ids=[c[0] for c in SEAM_CONFIGS])
def test_seam_fuzz_pictures_made_conformant_equal_the_oracle(oracle, name, mb_w, mb_h, n_pics, kw):
    rng = np.random.default_rng(sum(map(ord, name)) * 7919)
    slots = kw["slots"]
    frames = [seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if "smooth" in name else "noise") for _ in range(slots)]
    pictures = (seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=(i != 2), dst_slot=i % slots, **kw) for i in range(n_pics))
    coded, changed, census = run_chain(oracle, mb_w, mb_h, slots, frames, pictures, name)
    assert coded > 0 and census.stats["j"] > 0
    if kw["level_style"] == "small":
        assert changed < coded // 2


@pytest.mark.parametrize("name,mb_w,mb_h,n_pics,kw", wp_cfg.CONFIGS, ids=[c[0] for c in wp_cfg.CONFIGS])
def test_weighted_fuzz_pictures_made_conformant_equal_the_oracle(oracle, name, mb_w, mb_h, n_pics, kw):
    inputs = wp_cfg.config_inputs(name, mb_w, mb_h, n_pics, kw)
    frames = next(inputs)
    run_chain(oracle, mb_w, mb_h, kw["slots"], frames, inputs, name)


@pytest.mark.parametrize("name", sorted(ipcm_cfg.CONFIGS))
def test_ipcm_fuzz_pictures_made_conformant_equal_the_oracle(oracle, name):
    """the pictures of ipcm_seam_stim.prepare (the batch without an I picture), drawn as it draws them"""
    mb_w, mb_h, share, samples, kw = ipcm_cfg.CONFIGS[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 131)
    smooth = samples == "frame"
    n_pcm = 0
    for s in range(ipcm_cfg.S):
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if smooth else "noise")
        k = dict(kw)
        k.setdefault("level_style", "mixed"); k.setdefault("qp_mode", "random")
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=True, slots=ipcm_cfg.SLOTS, dst_slot=ipcm_cfg.DST, intra_share=0.15, **k)
        if smooth:
            pic.desc.alpha_c0_offset = pic.desc.beta_offset = 6
        pcm_fuzz.to_ipcm(rng, pic, share, samples=samples, src=f)
        n_pcm += int((pic.rec["mb_type"] == N.MB_IPCM).sum())
        run_chain(oracle, mb_w, mb_h, ipcm_cfg.SLOTS, [f] * ipcm_cfg.DST + [f], [pic], "%s stream %d" % (name, s))
    assert n_pcm > 0


def test_spec_recon_needs_no_oracle(monkeypatch):
    """the three modules name nothing of the oracle's binding, and a picture is reconstructed while loading the oracle is an error"""
    import ctypes
    from tests import oracle_bind
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ("spec_recon.py", "inter_checker.py", "residual_checker.py"):
        text = open(os.path.join(here, f)).read()
        assert "oracle_bind" not in text and "CDLL" not in text and "liboracle" not in text, f

    def refuse(*a, **k):
        raise AssertionError("the oracle was asked for")
    monkeypatch.setattr(oracle_bind, "load", refuse)
    monkeypatch.setattr(ctypes, "CDLL", refuse)
    rng = np.random.default_rng(11)
    spec = spec_recon.SpecRecon(5, 4, 3)
    for s in range(3):
        spec.store.write(s, seam_fuzz.random_frame(rng, 5, 4))
    kinds = set()
    for i in range(4):
        pic = seam_fuzz.make_picture(rng, 5, 4, p_picture=i != 3, b_picture=i == 1, n_ref=2, n_ref_l1=2, slots=3, dst_slot=i % 3, intra_share=0.3,
                                     explicit_wp="legal" if i == 2 else None)
        if i == 0:
            pcm_fuzz.to_ipcm(rng, pic, 0.2)
        residual_checker.make_conformant(pic)
        before = [p.copy() for p in spec.store[pic.desc.dst_slot]]
        out = spec.reconstruct(pic)
        assert any(not np.array_equal(a, b) for a, b in zip(out, before))
        kinds |= set(pic.rec["mb_type"].tolist())
    assert kinds >= {N.MB_I4x4, N.MB_I16x16, N.MB_IPCM, N.MB_P_L0, N.MB_B}


def test_out_of_range_pictures_are_refused():
    rng = np.random.default_rng(12)
    pic = seam_fuzz.make_picture(rng, 4, 3, level_style="wrap", n_ref=1, slots=2)
    spec = spec_recon.SpecRecon(4, 3, 2)
    with pytest.raises(residual_checker.OutOfRange):
        spec.reconstruct(pic)


DIGESTS = {"typical": "30400dbb7e0359da", "int16_wrap": "98293dd6eaa4e7e5", "mixed_levels_3refs": "8cba43c6a318bc6e", "two_qps_smooth": "38c1980ce58e14a8",
           "far_vectors": "e15ea646323c4a14", "quadrant_partitions_only": "40ea5e29f84de853"}


def test_a_seed_gives_the_picture_it_always_gave():
    """seam_fuzz.make_picture's draws, pinned (digests taken on the commit before the checkers of this file existed)"""
    for name, mb_w, mb_h, n_pics, kw in SEAM_CONFIGS[:6]:
        rng = np.random.default_rng(sum(map(ord, name)) * 7919)
        for s in range(kw["slots"]):
            seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if "smooth" in name else "noise")
        assert seam_fuzz.picture_digest(seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=True, dst_slot=0, **kw)) == DIGESTS[name], name
