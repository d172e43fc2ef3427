"""Explicit weighted prediction on the MI355X (H.264 8.4.2.3.2): the weighted generic class of k_mc_wp and the picture-based
boundary-strength test of weighted P pictures.

- Known-answer pictures built directly: P and B pictures whose quadrants predict from list 0, list 1 or both, from three
  reference frames with whole-sample vectors (windows inside and outside the picture), random denominators, weights and offsets
  plus the extremes that clip; checked against the 8.4.2.3.2 formulas in numpy.  Weighted and unweighted pictures share one
  reconstruct call at batch sizes 1, 7 and 256; the unweighted ones must come out as they do alone.
- Streams: a table of weight 2^denom and offset 0 changes nothing, so a --wp-identity stream (every phase class, residual,
  sub-8x8, slices, CABAC B pictures) decodes to the frames of the unweighted stream from the same seed.
"""

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, Parser, _native as N
from tests import seam_fuzz, synth_cases
from tests.hip_harness import compare, cli_bytes, planes_bytes, reconstructor

pytestmark = pytest.mark.gpu

REFS = 3                 # reference frames in slots 0..2, the picture goes to slot 3


def clip(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def weigh(p0, p1, use0, use1, e0, e1, d):
    """8.4.2.3.2 on int arrays; e = (weight, offset)"""
    p0, p1 = p0.astype(np.int64), p1.astype(np.int64)
    if use0 and use1:
        return clip(((p0 * e0[0] + p1 * e1[0] + (1 << d)) >> (d + 1)) + ((e0[1] + e1[1] + 1) >> 1))
    p, (w, o) = (p0, e0) if use0 else (p1, e1)
    return clip(((p * w + (1 << (d - 1))) >> d) + o) if d >= 1 else clip(p * w + o)


def block(plane, x, y, n):
    h, w = plane.shape
    ys = np.clip(np.arange(y, y + n), 0, h - 1)
    xs = np.clip(np.arange(x, x + n), 0, w - 1)
    return plane[np.ix_(ys, xs)]


def random_table(rng, is_b):
    d = [int(rng.integers(0, 8)), int(rng.integers(0, 8))]
    t = np.zeros((2, 16, 3, 2), np.int16)
    lo, hi = (-64, 63) if is_b else (-128, 127)
    for l in range(2):
        for i in range(16):
            for c in range(3):
                k = rng.integers(0, 6)
                w = [lo, hi, 1 << d[min(c, 1)], 0][k] if k < 4 else int(rng.integers(lo, hi + 1))
                if is_b:
                    w = min(max(w, lo), hi)
                o = int(rng.choice([-128, 127, 0, int(rng.integers(-128, 128))]))
                t[l, i, c] = (w, o)
    return d, t


def build(rng, mb_w, mb_h, is_b, weighted):
    pic = seam_fuzz.SeamPicture(mb_w, mb_h)
    d = pic.desc
    d.slice_type = N.SLICE_B if is_b else N.SLICE_P
    d.dst_slot, d.n_ref = REFS, REFS
    for i in range(REFS):
        d.ref_slot[i] = i
    if is_b:
        d.n_ref_l1 = REFS
        for i in range(REFS):
            d.ref_slot_l1[i] = (i + 1) % REFS
    pic.rec["mb_type"] = N.MB_B if is_b else N.MB_P_8x8
    pic.rec["qp"] = 26
    n = mb_w * mb_h
    mv = pic.mv.reshape(n, 16, 2)
    mv1 = pic.mv_l1.reshape(n, 16, 2)
    for m in range(n):
        for q in range(4):
            which = int(rng.integers(0, 3)) if is_b else 0           # 0 list 0, 1 list 1, 2 both
            r0 = int(rng.integers(0, REFS)) if which != 1 else -1
            r1 = int(rng.integers(0, REFS)) if which != 0 else -1
            pic.ref_idx[m * 4 + q] = r0
            pic.ref_idx_l1[m * 4 + q] = r1
            # whole chroma samples (multiples of 8 quarter-pels), up to 20 luma samples past the edges: clamped windows
            v0 = rng.integers(-10, 11, 2) * 8 if r0 >= 0 else (0, 0)
            v1 = rng.integers(-10, 11, 2) * 8 if r1 >= 0 else (0, 0)
            for b in (0, 1, 4, 5):
                k = (q >> 1) * 8 + (q & 1) * 2 + b
                mv[m, k] = v0
                mv1[m, k] = v1
    if weighted:
        den, tab = random_table(rng, is_b)
        d.explicit_wp = 1
        d.wp_log2_denom[0], d.wp_log2_denom[1] = den
        np.ctypeslib.as_array(d.wp)[:] = tab.reshape(-1)
    return pic.seal()


def expected(pic, frames):
    d = pic.desc
    is_b = d.slice_type == N.SLICE_B
    n = d.mb_w * d.mb_h
    mv, mv1 = pic.mv.reshape(n, 16, 2), pic.mv_l1.reshape(n, 16, 2)
    tab = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2).astype(np.int64)
    out = [np.zeros_like(f) for f in frames[0]]
    for m in range(n):
        mbx, mby = m % d.mb_w, m // d.mb_w
        for q in range(4):
            r0, r1 = int(pic.ref_idx[m * 4 + q]), int(pic.ref_idx_l1[m * 4 + q]) if is_b else -1
            k = (q >> 1) * 8 + (q & 1) * 2
            for c in range(3):
                s = 8 if c == 0 else 4
                x, y = mbx * 2 * s + (q & 1) * s, mby * 2 * s + (q >> 1) * s
                sh = 2 if c == 0 else 3
                p0 = block(frames[r0][c], x + (int(mv[m, k, 0]) >> sh), y + (int(mv[m, k, 1]) >> sh), s) if r0 >= 0 else None
                p1 = block(frames[d.ref_slot_l1[r1]][c], x + (int(mv1[m, k, 0]) >> sh), y + (int(mv1[m, k, 1]) >> sh), s) if r1 >= 0 else None
                if d.explicit_wp:
                    dd = d.wp_log2_denom[min(c, 1)]
                    e0 = tab[0, max(r0, 0), c]
                    e1 = tab[1, max(r1, 0), c]
                    v = weigh(p0 if p0 is not None else p1, p1 if p1 is not None else p0, r0 >= 0, r1 >= 0, e0, e1, dd)
                elif r0 >= 0 and r1 >= 0:
                    v = ((p0.astype(np.int64) + p1 + 1) >> 1).astype(np.uint8)
                else:
                    v = p0 if r0 >= 0 else p1
                out[c][y:y + s, x:x + s] = v
    return out


@pytest.mark.parametrize("batch", [1, 7, 256])
def test_known_answer_pictures_mixed_batches(lib, batch):
    rng = np.random.default_rng(4100 + batch)
    mb_w, mb_h = (5, 3) if batch < 256 else (2, 2)
    with reconstructor(lib, mb_w, mb_h, n_streams=batch, slots=REFS + 1, max_pictures=batch) as hip:
        shapes = [(mb_h * 16, mb_w * 16), (mb_h * 8, mb_w * 8), (mb_h * 8, mb_w * 8)]
        pics, frames = [], []
        for s in range(batch):
            fr = [[rng.integers(0, 256, sh, dtype=np.uint8) for sh in shapes] for _ in range(REFS)]
            for i, f in enumerate(fr):
                hip.write_frame(s, i, *f)
            is_b, weighted = bool(s & 2), (s % 3 != 1) if batch > 1 else True
            pics.append(build(rng, mb_w, mb_h, is_b, weighted))
            frames.append(fr)
        hip.upload(0, pics)
        hip.reconstruct(list(range(batch)), list(range(batch)))
        hip.sync()
        for s in range(batch):
            got = hip.read_frame(s, REFS)
            want = expected(pics[s], frames[s])
            compare(got, want, "stream %d (%s, weighted %d)" % (s, "B" if pics[s].desc.slice_type == N.SLICE_B else "P", pics[s].desc.explicit_wp))


def decode(lib, data):
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    slots = parser.slots
    parser.close()
    with reconstructor(lib, pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
        out = []
        for p in pics:
            hip.submit(0, p)
            out.append([a.copy() for a in hip.read_frame(0, p.desc.dst_slot)])
    return pics, out, slots


@pytest.mark.parametrize("args", [
    "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 81 --refs 2 --sub8x8 --slices 2 --coded 25 --maxlevel 8 --wp",
    "--mbw 7 --mbh 5 --frames 10 --seed 82 --refs 2 --bframes 2 --cabac --coded 25 --maxlevel 8 --wp --wp-bi",
    "--mbw 7 --mbh 5 --frames 10 --seed 83 --refs 3 --bframes 2 --temporal --coded 25 --maxlevel 8 --wp --wp-bi",
])
def test_identity_weights_decode_like_the_unweighted_stream(lib, tmp_path, args):
    base = args.replace(" --wp-bi", "").replace(" --wp", "")
    pa, plain, _ = decode(lib, synth_cases.write_stream(tmp_path, base, "plain"))
    pb, ident, _ = decode(lib, synth_cases.write_stream(tmp_path, args + " --wp-identity", "ident"))
    assert any(p.desc.explicit_wp for p in pb)
    assert len(plain) == len(ident)
    for k, (a, b) in enumerate(zip(plain, ident)):
        compare(a, b, "picture %d" % k)


def test_weighted_streams_decode_the_same_on_every_road(lib, tmp_path):
    """one weighted stream (duplicated list entries, loop filter on): per picture, upload vs the compact link format"""
    data = synth_cases.write_stream(tmp_path, "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 84 --refs 2 --wp --wp-dup --coded 25 --maxlevel 8", "dup")
    pics, frames, slots = decode(lib, data)
    assert any(p.desc.explicit_wp and p.desc.n_ref > 1 and p.desc.ref_slot[0] == p.desc.ref_slot[1] for p in pics)
    with reconstructor(lib, pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
        for k, p in enumerate(pics):
            compact = HipReconstructor.pack_compact(p, lib)
            hip.upload_compact(0, p, compact)
            hip.reconstruct([0], [0])
            got = hip.read_frame(0, p.desc.dst_slot)
            compare(got, frames[k], "picture %d" % k)


def test_duplicated_entries_loop_filter_against_oracle(lib, oracle, tmp_path):
    """--wp-dup puts one frame at list-0 indices 0 and 1 (with identity weights the prediction is the unweighted one): the loop
    filter must compare pictures (8.7.2.1), as the CPU oracle does on the picture's own indices - both agree, picture by picture,
    loop filter on."""
    from tests import oracle_bind
    data = synth_cases.write_stream(tmp_path, "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 85 --refs 2 --wp --wp-dup --wp-identity --coded 25 --maxlevel 8", "dupid")
    pics, frames, slots = decode(lib, data)
    store = oracle_bind.FrameStore(pics[0].mb_w, pics[0].mb_h, slots)
    changed = 0
    for k, p in enumerate(pics):
        d = p.desc
        for i, r in enumerate(p.ref_idx):
            if r > 0:
                first = [d.ref_slot[j] for j in range(d.n_ref)].index(d.ref_slot[r])
                changed += first != r
        want = oracle_bind.reconstruct(oracle, store, p)
        compare(frames[k], want, "picture %d" % k)
    assert changed > 0                                   # the stream does use the second index of a duplicated frame


def test_cli_decodes_a_weighted_stream_like_the_python_path(lib, tmp_path):
    """the drop-in API (p264_decoder_decode) behind the command-line decoder: the same frames"""
    args = "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 86 --refs 2 --sub8x8 --coded 25 --maxlevel 8 --wp --wp-dup"
    data = synth_cases.write_stream(tmp_path, args, "cli")
    pics, frames, _ = decode(lib, data)
    assert all(p.desc.explicit_wp for p in pics[1:])
    assert cli_bytes(tmp_path, data) == planes_bytes(frames)


@pytest.mark.parametrize("args", [
    # CAVLC P: three references, sub-8x8 partitions, two slices (residual, every phase class, real weights)
    "--mbw 10 --mbh 7 --frames 8 --gop 0 --seed 101 --refs 3 --mmco --sub8x8 --slices 2 --coded 25 --maxlevel 8 --wp",
    # CABAC I / P / B with explicit weights in both
    "--mbw 9 --mbh 6 --frames 10 --seed 102 --refs 2 --bframes 2 --cabac --coded 25 --maxlevel 8 --wp --wp-bi",
    # B pictures with temporal direct prediction and slices
    "--mbw 9 --mbh 6 --frames 10 --seed 103 --refs 3 --bframes 2 --temporal --slices 2 --coded 25 --maxlevel 8 --wp --wp-bi",
    # one frame at list-0 indices 0 and 1 with different weights, loop filter on
    "--mbw 10 --mbh 7 --frames 8 --gop 0 --seed 104 --refs 2 --coded 25 --maxlevel 8 --wp --wp-dup",
])
def test_weighted_streams_against_the_checker(lib, oracle, tmp_path, args):
    """HIP against tests/wp_checker.py (oracle_mc_* + the 8.4.2.3.2 formula, then the oracle's residual and loop filter),
    picture by picture"""
    from tests import wp_checker
    data = synth_cases.write_stream(tmp_path, args, "chk")
    pics, frames, slots = decode(lib, data)
    assert sum(p.desc.explicit_wp for p in pics) >= 3
    chk = wp_checker.WeightedChecker(oracle, pics[0].mb_w, pics[0].mb_h, slots)
    for k, p in enumerate(pics):
        want = chk.reconstruct(p)
        compare(frames[k], want, "picture %d (type %d, weighted %d)" % (k, p.desc.slice_type, p.desc.explicit_wp))
