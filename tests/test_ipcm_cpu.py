"""I_PCM macroblocks (H.264 7.3.5 / 8.3.5; the reference stops at them, decoder/macroblock.c:510-514) on the CPU side: the
checker's own check, the parser against the stream writer's record and against itself (CAVLC form = CABAC form), what the
streams contain, refusals, and the seam formats.  Every parser test fails without the feature (the parser refused the type)."""
import ctypes as C
import random

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, Parser, _native as N
from p264decoder_amd.recon import P264Error
from tests import oracle_bind, pcm_checker, pcm_fuzz, seam_fuzz, synth_cases
from tests.stream_args import IPCM_STREAMS as STREAMS

IPCM_MASK = 0x00000fff
EINVAL = -1                                              # P264HIP_EINVAL
FIELDS = ("mb", "mv", "ref_idx", "i4modes", "coefs")


def read_dump(path):
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        n = int.from_bytes(raw[at:at + 4], "little"); at += 4
        pic = []
        for _ in range(n):
            pic.append((int.from_bytes(raw[at:at + 4], "little"), raw[at + 4:at + 388])); at += 388
        out.append(pic)
    return out


# ---- the checker checks itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["P", "B", "I"])
def test_checker_gives_back_the_oracle_picture_before_the_loop_filter(oracle, kind):
    """pictures WITHOUT I_PCM through oracle_reconstruct_nodeblock; then a share of their macroblocks, intra and inter, become
    I_PCM records carrying exactly the samples the oracle produced there: steps 1 - 2 of the checker must give the same picture,
    byte for byte.  (Behind the loop filter they differ by design: QP 0.)"""
    rng = np.random.default_rng({"P": 11, "B": 12, "I": 13}[kind])
    mb_w, mb_h, slots = 7, 6, 3
    n_pcm = 0
    for trial in range(8):
        store = oracle_bind.FrameStore(mb_w, mb_h, slots)
        chk = pcm_checker.PcmChecker(oracle, mb_w, mb_h, slots)
        for s in range(slots):
            f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if trial & 1 else "noise")
            for a, b, c in zip(store[s], chk.store[s], f):
                a[:] = c; b[:] = c
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=kind != "I", b_picture=kind == "B", n_ref=2, n_ref_l1=2, slots=slots, dst_slot=2,
                                     level_style="mixed", qp_mode="random", slices=1 + trial % 3, intra_share=0.3)
        want = [a.copy() for a in oracle_bind.reconstruct(oracle, store, pic, deblock=False)]
        chosen = rng.random(pic.n_mb) < 0.3
        n_pcm += int(chosen.sum())
        pcm_fuzz.to_ipcm(rng, pic, 0, samples="frame", src=want, chosen=chosen, noise=0)
        got = chk.nodeblock(pic)
        for plane, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), "%s trial %d plane %d" % (kind, trial, plane)
        chk.reconstruct(pic)                                  # (step 3 runs on records of type 2 / qp 0)
    assert n_pcm > 40


def test_checker_refuses_a_full_list():
    oracle = oracle_bind.load()
    rng = np.random.default_rng(5)
    pic = seam_fuzz.make_picture(rng, 3, 2, n_ref=1, slots=2, dst_slot=0)
    pcm_fuzz.to_ipcm(rng, pic, 1.0)
    pic.desc.n_ref = 16
    with pytest.raises(ValueError, match="no room"):
        pcm_checker.PcmChecker(oracle, 3, 2, 2).nodeblock(pic)


def test_road_model_of_the_sparse_path():
    rng = np.random.default_rng(3)
    pic = seam_fuzz.make_picture(rng, 6, 4, n_ref=1, slots=2, dst_slot=0, intra_share=0.0)
    m = np.zeros(24, bool); m[[0, 1, 2, 6, 7, 8, 12, 13, 14, 5]] = True     # a 3x3 cluster and a lone macroblock
    pcm_fuzz.to_ipcm(rng, pic, 0, chosen=m)
    road = pcm_checker.sparse_roads(pic).reshape(4, 6)
    assert road[0, 0] == 0 and road[0, 5] == 0 and road[0, 1] == 1 and road[1, 0] == 2 and road[1, 1] == 2 and road[2, 2] == 2 and road[3, 3] == -1


# ---- the parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ip_baseline", "b_spatial", "slices3", "style_flat"])
@pytest.mark.parametrize("cabac", [False, True])
def test_parser_finds_the_writers_samples(lib, tmp_path, name, cabac):
    dump = tmp_path / "pcm.bin"
    data = synth_cases.write_stream(tmp_path, STREAMS[name] + " --dump-pcm %s" % dump + (" --cabac" if cabac else ""), "s")
    pics = Parser(quiet=True, lib=lib).parse_stream(data)
    want = read_dump(str(dump))
    assert len(pics) == len(want) and sum(len(w) for w in want) > 20
    for i, (p, w) in enumerate(zip(pics, want)):
        got = p.ipcm_macroblocks()
        assert [m for m, _ in got] == [m for m, _ in w], "picture %d: which macroblocks are I_PCM" % i
        for (m, s), (_, ws) in zip(got, w):
            assert s.tobytes() == ws, "picture %d macroblock %d: samples" % (i, m)
        r = p.mb_records()
        pcm = r["mb_type"] == N.MB_IPCM
        assert (r["qp"][pcm] == 0).all() and (r["coef_mask"][pcm] == IPCM_MASK).all() and (r["cbp"][pcm] == 0).all() and (r["intra_modes"][pcm] == 0).all()
        assert (p.i4modes.reshape(-1, 16)[pcm] == 2).all() and (p.ref_idx.reshape(-1, 4)[pcm] == -1).all() and not p.mv.reshape(-1, 32)[pcm].any()
        assert (r["coef_index"][pcm].astype(np.int64) + 12 <= p.desc.n_coef_blocks).all()


@pytest.mark.parametrize("name", list(STREAMS))
def test_cavlc_and_cabac_forms_of_ipcm_streams_parse_to_the_same_pictures(lib, tmp_path, name):
    args = STREAMS[name]
    a = Parser(quiet=True, strict=True, lib=lib).parse_stream(synth_cases.write_stream(tmp_path, args, "cavlc"))
    c = Parser(quiet=True, lib=lib).parse_stream(synth_cases.write_stream(tmp_path, args + " --cabac", "cabac"))
    assert len(a) == len(c) == int(args.split("--frames ")[1].split()[0])
    n_pcm = 0
    for i, (p, q) in enumerate(zip(a, c)):
        assert p.desc.slice_type == q.desc.slice_type and p.desc.n_coef_blocks == q.desc.n_coef_blocks
        for f in FIELDS:
            assert np.array_equal(getattr(p, f), getattr(q, f)), "picture %d: %s differs" % (i, f)
        if p.desc.slice_type == N.SLICE_B:
            assert np.array_equal(p.mv_l1, q.mv_l1) and np.array_equal(p.ref_idx_l1, q.ref_idx_l1), "picture %d: list-1 motion differs" % i
        n_pcm += len(p.ipcm_macroblocks())
    assert n_pcm > 20
    if name == "all_ipcm":
        assert all((p.mb_records()["mb_type"] == N.MB_IPCM).all() for p in a)


def test_the_qp_chain_passes_through_an_ipcm_macroblock(lib, tmp_path):
    """no mb_qp_delta is coded for I_PCM: a macroblock without residual syntax right behind one carries the QP the chain had in
    front of it (conformant chain), and the I_PCM record itself says 0"""
    pics = Parser(quiet=True, strict=True, lib=lib).parse_stream(synth_cases.write_stream(tmp_path, STREAMS["qp_delta"], "q"))
    seen = 0
    for p in pics:
        r = p.mb_records()
        for m in range(2, p.n_mb):
            if r["mb_type"][m - 1] == N.MB_IPCM and r["mb_type"][m - 2] != N.MB_IPCM and r["mb_type"][m] not in (N.MB_IPCM, N.MB_I16x16) and r["cbp"][m] == 0:
                assert r["qp"][m] == r["qp"][m - 2], "macroblock %d" % m
                seen += 1
    assert seen > 3
    assert len({int(q) for p in pics for q in p.mb_records()["qp"]}) > 6


def test_what_the_streams_contain(lib, tmp_path):
    kinds, corners, nc16, epb = set(), set(), 0, 0
    for name in ("ip_baseline", "slices3", "style_flat", "i_only", "refs2_sub8x8"):
        data = synth_cases.write_stream(tmp_path, STREAMS[name], "c")
        if name == "style_flat":
            plain = synth_cases.write_stream(tmp_path, STREAMS[name].replace("--ipcm-style flat", ""), "p")
            epb = data.count(b"\x00\x00\x03") - plain.count(b"\x00\x00\x03")
        for p in Parser(quiet=True, lib=lib).parse_stream(data):
            kinds |= pcm_fuzz.neighbour_kinds(p)
            r = p.mb_records()
            w, h = p.mb_w, p.mb_h
            for k, m in enumerate((0, w - 1, (h - 1) * w, h * w - 1)):
                if r["mb_type"][m] == N.MB_IPCM:
                    corners.add(k)
            for m in np.flatnonzero((r["mb_type"] != N.MB_IPCM) & ((r["cbp"] & 15) != 0)):
                if (r["avail"][m] & N.AVAIL_LEFT and r["mb_type"][m - 1] == N.MB_IPCM) or (r["avail"][m] & N.AVAIL_TOP and r["mb_type"][m - w] == N.MB_IPCM):
                    nc16 += 1                              # (its first coded luma block's nC counts a neighbour's 16)
    want = {(d, k) for d in ("left", "top", "topleft", "topright") for k in ("i4", "i16", "ipcm", "inter")}
    assert kinds == want, "missing neighbour combinations: %s" % sorted(want - kinds)
    assert corners == {0, 1, 2, 3}
    assert nc16 > 10
    assert epb > 20, "no emulation-prevention bytes inside the sample data"


def test_a_picture_of_nothing_but_ipcm_outgrows_the_levels_section(lib, tmp_path):
    """twelve blocks per macroblock against a section of eight: coef_reserve takes it"""
    pics = Parser(quiet=True, lib=lib).parse_stream(synth_cases.write_stream(tmp_path, "--mbw 20 --mbh 15 --frames 3 --gop 0 --seed 311 --ipcm 100", "big"))
    assert len(pics) == 3 and all(p.desc.n_coef_blocks == 12 * 300 for p in pics)
    dump = [(m, s) for m, s in pics[2].ipcm_macroblocks()]
    assert [m for m, _ in dump] == list(range(300))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def first_slice_at(data):
    at = 0
    while True:
        at = data.index(b"\x00\x00\x00\x01", at) + 4
        if data[at] & 31 in (1, 5):
            return at


@pytest.mark.parametrize("cabac", [False, True])
def test_a_slice_that_ends_inside_the_samples_is_an_error(lib, tmp_path, capfd, cabac):
    data = synth_cases.write_stream(tmp_path, "--mbw 4 --mbh 3 --frames 1 --seed 312 --ipcm 100" + (" --cabac" if cabac else ""), "t")
    at = first_slice_at(data)
    for cut in (at + 40, at + 200, at + 380):              # (all inside the first macroblock's 384 bytes)
        capfd.readouterr()
        with pytest.raises(P264Error):
            Parser(quiet=True, lib=lib).parse_stream(data[:cut])
        assert "macroblock overruns the slice data" in capfd.readouterr().err, "cut at %d" % cut


@pytest.mark.parametrize("cabac", [False, True])
def test_a_nonzero_alignment_bit_is_an_error(lib, tmp_path, capfd, cabac):
    """the bits between the macroblock type (CABAC: the encoder's flush) and the first sample byte: flipping one of the bits in
    front of the first macroblock's samples must be refused with the parser's message (which bit is an alignment bit depends on
    the slice header's length: every bit of the bytes in front of the samples is tried, one at a time)"""
    data = synth_cases.write_stream(tmp_path, "--mbw 4 --mbh 3 --frames 1 --seed 313 --qp 30 --ipcm 100 --dump-pcm %s" % (tmp_path / "d.bin") + (" --cabac" if cabac else ""), "t")
    first = read_dump(str(tmp_path / "d.bin"))[0][0][1]
    at = data.index(first[:16])                             # (noise samples: no emulation prevention in the first sixteen)
    hits = 0
    for bit in range(16):
        d = bytearray(data)
        d[at - 1 - (bit >> 3)] ^= 1 << (bit & 7)
        capfd.readouterr()
        try:
            Parser(quiet=True, lib=lib).parse_stream(bytes(d))
        except P264Error:
            pass
        hits += "pcm_alignment_zero_bit is not zero" in capfd.readouterr().err
    assert hits >= 1


@pytest.mark.parametrize("cabac", [False, True])
def test_damaged_ipcm_streams_do_not_crash(lib, tmp_path, cabac):
    data = synth_cases.write_stream(tmp_path, STREAMS["b_spatial"] + (" --cabac" if cabac else ""), "c")
    random.seed(11 + cabac)
    ok = bad = 0
    for trial in range(100):
        d = bytearray(data)
        for _ in range(random.randrange(1, 12)):
            d[random.randrange(30, len(d))] = random.randrange(256)
        try:
            Parser(quiet=True, lib=lib).parse_stream(bytes(d[:random.randrange(60, len(d))]))
            ok += 1
        except P264Error:
            bad += 1
    assert ok + bad == 100 and bad > 0


# ---- the seam formats --------------------------------------------------------------------------------------------------------
def seam_pictures(rng):
    for k, (kind, share) in enumerate([("P", 0.02), ("P", 0.3), ("P", 1.0), ("B", 0.3), ("B", 1.0), ("I", 0.3), ("I", 1.0), ("P", 0.6), ("B", 0.05)]):
        pic = seam_fuzz.make_picture(rng, 9, 6, p_picture=kind != "I", b_picture=kind == "B", n_ref=2, n_ref_l1=2, slots=3, dst_slot=2, level_style="mixed",
                                     slices=1 + k % 3, intra_share=0.3)
        yield kind, share, pcm_fuzz.to_ipcm(rng, pic, share, samples=("noise", "extremes")[k & 1])


def test_slot_layout_and_compact_format_carry_ipcm_pictures(lib):
    rng = np.random.default_rng(77)
    for kind, share, pic in seam_pictures(rng):
        d = pic.desc
        packed = HipReconstructor.pack(pic, lib)
        view = N.Picture()
        assert lib.p264hip_unpack_input(C.byref(d), packed.ctypes.data, packed.size, C.byref(view)) == 0
        n = pic.n_mb
        assert np.array_equal(np.ctypeslib.as_array(C.cast(view.mb, C.POINTER(C.c_uint8)), (n * 16,)), pic.rec.view(np.uint8))
        assert np.array_equal(np.ctypeslib.as_array(view.coefs, (d.n_coef_blocks * 16,)), pic.coefs)
        assert np.array_equal(np.ctypeslib.as_array(view.mv, (n * 32,)), pic.mv) and np.array_equal(np.ctypeslib.as_array(view.i4modes, (n * 16,)), pic.i4modes)
        comp = HipReconstructor.pack_compact(pic, lib)
        assert lib.p264hip_compact_check(C.byref(d), comp.ctypes.data, comp.size) == 0
        assert np.array_equal(HipReconstructor.expand_compact(pic, comp, lib), packed), "%s picture, share %.2f: expand(pack_compact) != pack_input" % (kind, share)
        assert int((pic.rec["mb_type"] == N.MB_IPCM).sum()) >= share * n * 0.5


@pytest.mark.parametrize("what", ["mask_7ff", "mask_1fff", "past_the_end"])
def test_host_checks_refuse_a_bad_ipcm_record(lib, what):
    rng = np.random.default_rng(78)
    pic = pcm_fuzz.to_ipcm(rng, seam_fuzz.make_picture(rng, 6, 5, n_ref=1, slots=2, dst_slot=0), 0.4)
    good_c = HipReconstructor.pack_compact(pic, lib)
    m = int(np.flatnonzero(pic.rec["mb_type"] == N.MB_IPCM)[-1])             # the picture's last I_PCM macroblock
    if what == "past_the_end":
        pic.desc.n_coef_blocks = int(pic.rec["coef_index"][m]) + 11           # (host functions only: nothing of this goes near a launch)
        hdr_fix = lambda c: c.view(np.uint32).__setitem__(2, pic.desc.n_coef_blocks)
    else:
        pic.rec["coef_mask"][m] = 0x7ff if what == "mask_7ff" else 0x1fff
        hdr_fix = lambda c: None
    buf = np.zeros(1 << 20, np.uint8)
    assert lib.p264hip_pack_input(C.byref(pic.desc), buf.ctypes.data, buf.size) == EINVAL
    assert lib.p264hip_pack_compact(C.byref(pic.desc), buf.ctypes.data, buf.size) == EINVAL
    # the same record inside an otherwise good compact block (records travel verbatim in it)
    hdr = np.frombuffer(good_c[:128].tobytes(), np.uint32)
    bad = good_c.copy()
    off_rec = int(hdr[5])
    if what == "past_the_end":
        hdr_fix(bad)
    else:
        bad[off_rec + 16 * m + 4:off_rec + 16 * m + 8] = np.frombuffer(np.uint32(pic.rec["coef_mask"][m]).tobytes(), np.uint8)
    assert lib.p264hip_compact_check(C.byref(pic.desc), bad.ctypes.data, bad.size) != 0
