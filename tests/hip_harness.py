"""What the GPU tests share: a HipReconstructor that closes on every exit path, the four roads into an input slot, batches of
distinct pictures, the refusals of the device roads, the stream path (parser + submit, drop-in decoder, command-line decoder)
and the one plane comparer.  Plain functions and context managers, no fixtures; nothing here decides what a picture should look
like - that stays with the checkers and the stimulus modules."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Decoder, HipReconstructor, Parser, build as _build
from p264decoder_amd.recon import P264Error

CLI = os.path.join(os.path.dirname(_build.__file__), "tools", "p264decoder_amd")
ROADS = ("upload", "packed", "compact", "commit")


# ---- comparing planes ----------------------------------------------------------------------------------------------------------
def records_of(pic):
    """the macroblock records of a seam_fuzz.SeamPicture (.rec) or a recon.ParsedPicture (.mb_records())"""
    return pic.rec if hasattr(pic, "rec") else pic.mb_records()


def first_difference(got, want, what, pic=None):
    """None, or one message about the first plane that differs: how many samples, the first in raster order, its macroblock
    (with pic: that record's type, availability, QP, mask and first vector) and both values"""
    for plane, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return "%s plane %d: shape %s, expected %s" % (what, plane, a.shape, b.shape)
        if np.array_equal(a, b):
            continue
        ys, xs = np.nonzero(a != b)
        y, x, s = int(ys[0]), int(xs[0]), 16 if plane == 0 else 8
        m = (y // s) * -(-b.shape[1] // s) + x // s
        about = ""
        if pic is not None:
            r = records_of(pic)[m]
            about = " type %d avail %d qp %d mask %#x vector %s" % (r["mb_type"], r["avail"], r["qp"], r["coef_mask"], pic.mv[m * 32:m * 32 + 2].tolist())
        return "%s plane %d: %d samples differ, first (y=%d, x=%d) macroblock %d%s: got %d want %d" % (
            what, plane, len(ys), y, x, m, about, a[y, x], b[y, x])
    return None


def differences(got, want, what, pic=None):
    """[] or [the message]: for tests that collect over many pictures and assert once"""
    d = first_difference(got, want, what, pic)
    return [d] if d else []


def compare(got, want, what, pic=None):
    d = first_difference(got, want, what, pic)
    if d:
        pytest.fail(d)


def compare_pictures(got, want, what, crop=False):
    """two lists of pictures, one by one; crop: the expected plane's shape out of the top left of a padded plane"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if crop:
            g = [np.asarray(a)[:b.shape[0], :b.shape[1]] for a, b in zip(g, w)]
        compare(g, w, "%s picture %d" % (what, i))


# ---- the context, its frames and its input slots -------------------------------------------------------------------------------
@contextlib.contextmanager
def reconstructor(lib, mb_w, mb_h, **kw):
    hip = HipReconstructor(mb_w, mb_h, lib=lib, **kw)
    try:
        yield hip
    finally:
        hip.close()


def load_frames(hip, stream, frames):
    """write_frame for {slot: (y, u, v)} or [(y, u, v)] (slot = index)"""
    for slot, f in frames.items() if isinstance(frames, dict) else enumerate(frames):
        hip.write_frame(stream, slot, *f)


def put(hip, lib, slot, pic, road):
    """the picture into an input slot by one of ROADS (the context keeps packed and compact blocks referenced until its sync)"""
    if road == "upload":
        hip.upload(slot, [pic])
    elif road == "packed":
        hip.upload_packed(slot, pic, hip.pack(pic, lib))
    elif road == "compact":
        hip.upload_compact(slot, pic, hip.pack_compact(pic, lib))
    elif road == "commit":
        blk = hip.pack(pic, lib)
        dev, n = hip.input_reserve(slot, pic)
        assert n == blk.size and lib.p264hip_copy_to_device(dev, blk.ctypes.data, n) == 0
        hip.input_commit(slot)
    else:
        raise ValueError("no road %r" % (road,))


def through_roads(hip, lib, pic, want, what, roads):
    """the picture through each road into input slot 0 of stream 0: the same bytes every time"""
    dst = pic.desc.dst_slot
    blank = [np.zeros_like(a) for a in want]
    for road in roads:
        hip.write_frame(0, dst, *blank)           # (a road that wrote nothing cannot pass on the road before's output)
        put(hip, lib, 0, pic, road)
        hip.reconstruct([0], [0])
        compare(hip.read_frame(0, dst), want, "%s (%s)" % (what, road), pic)
    hip.sync()


def refused_on_device_roads(lib, hip, pic, good_block, mutations):
    """per (macroblock, field, value, the descriptor's transform_8x8): p264hip_upload refuses the record on the host, and behind
    reserve / copy / commit p264hip_reconstruct refuses it on the device; the picture is as it was afterwards"""
    rec, t8_keep = records_of(pic), int(pic.desc.transform_8x8)
    for m, field, value, t8 in mutations:
        keep = rec[field][m]
        rec[field][m], pic.desc.transform_8x8 = value, t8
        try:
            with pytest.raises(P264Error):                      # p264hip_upload checks on the host
                hip.upload(1, [pic])
            bad = good_block.copy()
            bad[16 * m:16 * m + 16] = np.frombuffer(rec[m:m + 1].tobytes(), np.uint8)
            dev, n = hip.input_reserve(0, pic)                  # reserve / commit: the check runs on the device
            assert n == bad.size and lib.p264hip_copy_to_device(dev, bad.ctypes.data, n) == 0
            hip.input_commit(0)
            with pytest.raises(P264Error):
                hip.reconstruct([0], [0])
        finally:
            rec[field][m], pic.desc.transform_8x8 = keep, t8_keep


# ---- stimuli (.pic, .frames, .name) against a spec model -----------------------------------------------------------------------
def expect(stim, recon_class, slots):
    """[y, u, v] of the stimulus by a fresh spec store with its frames written"""
    spec = recon_class(stim.pic.mb_w, stim.pic.mb_h, slots)
    for slot, f in stim.frames.items():
        spec.store.write(slot, f)
    return [p.copy() for p in spec.reconstruct(stim.pic)]


def by_size(cases):
    sizes = {}
    for st, want in cases:
        sizes.setdefault((st.pic.mb_w, st.pic.mb_h), []).append((st, want))
    return sizes


def batches_of(cases, n):
    """consecutive batches of n (stimulus, expected planes), the last one filled up from the front; n distinct pictures each"""
    for at in range(0, len(cases), n):
        batch = [cases[(at + k) % len(cases)] for k in range(n)]
        assert len({id(st.pic) for st, _ in batch}) == n
        yield batch


def submit_each(lib, cases, slots, probe=None):
    """every case through p264hip_submit, one context per picture size; probe(hip, stim) after each submit.  Returns (the
    differences, the stimuli sent)"""
    bad, sent = [], []
    for (mb_w, mb_h), same_size in by_size(cases).items():
        with reconstructor(lib, mb_w, mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
            for st, want in same_size:
                load_frames(hip, 0, st.frames)
                hip.submit(0, st.pic)
                if probe:
                    probe(hip, st)
                bad += differences(hip.read_frame(0, st.pic.desc.dst_slot), want, st.name, st.pic)
                sent.append(st)
    return bad, sent


def run_batches(lib, cases, n=3, road="upload", slots=3, probe=None):
    """the cases (one picture size) in batches of n distinct pictures, one stream each.  Returns (the differences, the stimuli
    sent, per batch what probe(hip, batch) returned)"""
    (mb_w, mb_h), = by_size(cases)
    bad, sent, probed = [], [], []
    with reconstructor(lib, mb_w, mb_h, n_streams=n, slots=slots, max_pictures=n) as hip:
        for batch in batches_of(cases, n):
            for k, (st, _) in enumerate(batch):
                load_frames(hip, k, st.frames)
            if road == "upload":
                hip.upload(0, [st.pic for st, _ in batch])
            else:
                for k, (st, _) in enumerate(batch):
                    put(hip, lib, k, st.pic, road)
            hip.reconstruct(list(range(n)), list(range(n)))
            if probe:
                probed.append(probe(hip, batch))
            for k, (st, want) in enumerate(batch):
                bad += differences(hip.read_frame(k, st.pic.desc.dst_slot), want, "%s (stream %d of a batch, %s)" % (st.name, k, road), st.pic)
                sent.append(st)
    return bad, sent, probed


# ---- a whole stream ------------------------------------------------------------------------------------------------------------
def decode_both(oracle, lib, data, limit=None):
    """every picture of a stream through tests/intra_checker.py and through the oracle (with pcm_checker's composition for I_PCM
    and explicit weights: oracle_reconstruct itself without them), each with its own frame store; returns the parsed pictures,
    how many of them differ, the first difference and the intra checker"""
    from tests import intra_checker, pcm_checker
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data, limit=limit) if limit else parser.parse_stream(data)
    chk = intra_checker.IntraChecker(oracle, pics[0].mb_w, pics[0].mb_h, parser.slots)
    ref = pcm_checker.PcmChecker(oracle, pics[0].mb_w, pics[0].mb_h, parser.slots)
    bad = []
    for i, p in enumerate(pics):
        bad += differences(chk.reconstruct(p), ref.reconstruct(p), "picture %d" % i, p)
    return pics, len(bad), bad[0] if bad else None, chk


def parse_and_expect(lib, data, make_checker, **parser_kw):
    """(the parser's pictures, its slots, per picture [y, u, v] by make_checker(mb_w, mb_h, slots) run picture after picture on its
    own frame store, the checker)"""
    parser = Parser(quiet=True, lib=lib, **parser_kw)
    pics = parser.parse_stream(data)
    checker = make_checker(pics[0].mb_w, pics[0].mb_h, parser.slots)
    return pics, parser.slots, [[a.copy() for a in checker.reconstruct(p)] for p in pics], checker


def submit_stream(lib, pics, slots, want, what, probe=None):
    """picture after picture through p264hip_submit on one stream; probe(hip, i, picture) after each submit"""
    with reconstructor(lib, pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
        for i, (p, w) in enumerate(zip(pics, want)):
            hip.submit(0, p)
            if probe:
                probe(hip, i, p)
            compare(hip.read_frame(0, p.desc.dst_slot), w, "%s picture %d" % (what, i), p)


def dropin_pictures(lib, data):
    """[[y, u, v]] of the stream by the drop-in decoder, decode order"""
    dec = Decoder(lib=lib)
    try:
        return [[np.array(a) for a in pic] for pic in dec.decode_annexb(data)]
    finally:
        dec.close()


def cli_bytes(tmp_path, data):
    """what the command-line decoder writes for the stream"""
    src, out = tmp_path / "in.264", tmp_path / "out.yuv"
    src.write_bytes(data)
    r = subprocess.run([CLI, "-d", str(src), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


def planes_bytes(want):
    return b"".join(np.ascontiguousarray(pl).tobytes() for f in want for pl in f)
