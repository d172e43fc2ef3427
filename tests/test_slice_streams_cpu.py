"""Slices of one picture that differ in their reference lists or their loop-filter offsets, through the host parser (no device):
the parse against the writer's own record (tests/slice_streams.py), slices that agree against digests of the commit before
(tests/golden/sliced_streams_parse.json), explicit weights with per-slice lists, what stays refused, and the packed / compact
forms of parsed pictures whose records carry deltas.  The streams of the first test were refused before (P264Error: "per-slice
deblocking offsets unsupported" / "slices of one picture with different reference lists unsupported")."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, Parser, _native as N
from p264decoder_amd.recon import P264Error
from tests import slice_streams as ss
from tests import synth_cases
from tests.tools.bitwriter import BitWriter


@pytest.mark.parametrize("name", list(ss.STREAMS))
def test_parser_against_the_writers_record(lib, tmp_path, name):
    args = ss.STREAMS[name]
    data, dump = ss.make(tmp_path, args)
    parser, pics = ss.parse(lib, data)
    assert len(pics) == int(args.split("--frames ")[1].split()[0])
    seen = ss.check_against_dump(pics, dump)
    assert seen["quadrants"] > 200
    if "--slice-deblock" in args:
        assert seen["pics_offsets_differ"] >= 3 and seen["pics_with_deltas"] >= 3 and seen["idc1_slices"] >= 1, seen
    else:
        assert not seen["pics_with_deltas"]
    if "--slice-lists" in args:
        assert seen["pics_lists_differ"] >= 3, seen
    # the descriptor keeps the offsets of the first slice that filters: -6 .. 6, and every sum of descriptor and delta as well
    for p in pics:
        assert -6 <= p.desc.alpha_c0_offset <= 6 and -6 <= p.desc.beta_offset <= 6


def test_the_streams_together_cover_the_cases(lib, tmp_path):
    """lists that grow past the first slice's, override lengths that differ inside a picture, in P and B, CAVLC and CABAC"""
    tot = {}
    for name in ("p_cavlc_4_sub8x8", "p_cabac_3", "b_cavlc_temporal_4", "b_cabac_spatial_2"):
        data, dump = ss.make(tmp_path, ss.STREAMS[name])
        seen = ss.check_against_dump(ss.parse(lib, data)[1], dump)
        assert seen["lists_grew"] >= 1 and seen["lengths_differ"] >= 1, (name, seen)
        for k, v in seen.items():
            tot[k] = tot.get(k, 0) + v
    assert tot["pics_lists_differ"] > 30 and tot["pics_offsets_differ"] > 20


def test_slices_that_agree_parse_to_what_they_did(lib):
    """the existing sliced streams: descriptors and arrays byte for byte what the commit before gave (digests recorded there)"""
    want = json.load(open(os.path.join(synth_cases.GOLDEN, "sliced_streams_parse.json")))
    assert sorted(want) == sorted(ss.AGREEING)
    for name, args in ss.AGREEING.items():
        pics = Parser(quiet=True, lib=lib).parse_stream(open(synth_cases.generate(args), "rb").read())
        assert ss.parse_digest(pics) == want[name], name
        assert not any(p.mb_records()["flags"].any() for p in pics)


# ---- explicit weights -------------------------------------------------------------------------------------------------------------
WP_STREAMS = {
    "p_cavlc": "--mbw 8 --mbh 6 --frames 10 --gop 10 --seed 121 --refs 2 --slices 3 --wp --coded 15 --maxlevel 6 --slice-lists",
    "b_cabac": "--mbw 8 --mbh 6 --frames 13 --seed 122 --refs 3 --bframes 2 --slices 3 --wp --wp-bi --cabac --coded 10 --maxlevel 6 --slice-lists --slice-deblock",
}


@pytest.mark.parametrize("name", list(WP_STREAMS))
def test_explicit_weights_with_per_slice_lists(lib, tmp_path, name):
    """every slice's entry (picture, weights of Y, Cb, Cr) is an entry of the picture's canonical list and table; the macroblocks of
    the slice name only such entries"""
    wp = str(tmp_path / "s.wp")
    data, dump = ss.make(tmp_path, WP_STREAMS[name], ["--dump-wp", wp])
    tables = np.fromfile(wp, dtype=np.int16).reshape(-1, 3 + 2 * 16 * 3 * 2)
    parser, pics = ss.parse(lib, data)
    ss.check_against_dump(pics, dump)
    recs = ss.records(dump, pics[0].n_mb)
    slot_pic, merged, grew = {}, 0, 0
    for i, (p, (sl, idc, alpha, beta, qpic, lists), t) in enumerate(zip(pics, recs, tables)):
        d = p.desc
        assert bool(d.explicit_wp) == bool(t[0]), i
        if d.explicit_wp:
            tab = t[3:].reshape(2, 16, 3, 2)
            got = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2)
            coded = [pair for pair in lists if pair[0]]
            for X, (slots, n_list) in enumerate(((d.ref_slot, d.n_ref), (d.ref_slot_l1, d.n_ref_l1))):
                if X == 1 and d.slice_type != N.SLICE_B:
                    continue
                canon = {(slot_pic[int(slots[j])], got[X, j].tobytes()) for j in range(n_list)}
                wanted = set()
                for s_no, pair in enumerate(coded):
                    mine = {(pic, tab[X, k].tobytes()) for k, pic in enumerate(pair[X])}
                    assert mine <= canon, "picture %d slice %d list %d: an entry of the slice is not in the picture's table" % (i, s_no, X)
                    wanted |= mine
                assert wanted == canon
                grew += n_list > len(coded[0][X])
                # every quadrant: the canonical entry it names is one of ITS slice's (picture, weights) pairs
                idx = p.ref_idx if X == 0 else p.ref_idx_l1
                slices = sorted(set(sl.tolist()))
                for m in range(p.n_mb):
                    pair = lists[slices.index(int(sl[m]))]
                    mine = {(pic, tab[X, k].tobytes()) for k, pic in enumerate(pair[X])}
                    for q in range(4):
                        r = int(idx[m * 4 + q])
                        if r >= 0 and p.mb_records()["mb_type"][m] > N.MB_IPCM:
                            assert (slot_pic[int(slots[r])], got[X, r].tobytes()) in mine, (i, m, q, X)
                            merged += 1
        if d.slice_type != N.SLICE_B:
            slot_pic[int(d.dst_slot)] = i
    assert merged > 300 and grew >= 2, (merged, grew)


def test_more_than_sixteen_entries_are_refused(lib, tmp_path, capfd):
    """three P slices that list four frames twice, each with its own eight weights and rotated by one: 24 (frame, weights) entries"""
    args = "--mbw 6 --mbh 5 --frames 9 --seed 123 --refs 4 --bframes 1 --slices 3 --wp --coded 10 --maxlevel 6 --slice-lists-many"
    data, _ = ss.make(tmp_path, args)
    with pytest.raises(P264Error):
        ss.parse(lib, data)
    assert "more than 16 entries in reference list 0" in capfd.readouterr().err
    # two such slices fit: sixteen entries
    data, dump = ss.make(tmp_path, args.replace("--slices 3", "--slices 2"))
    parser, pics = ss.parse(lib, data)
    ss.check_against_dump(pics, dump)
    assert max(p.desc.n_ref for p in pics) == 16


def test_what_stays_refused(lib, tmp_path, capfd):
    """per-slice weight tables; P and B slices in one picture"""
    data = synth_cases.write_stream(tmp_path, "--mbw 6 --mbh 4 --frames 3 --gop 0 --seed 77 --wp --slices 2 --wp-slice-differ", "r")
    with pytest.raises(P264Error):
        Parser(quiet=True, lib=lib).parse_stream(data)
    assert "slices of one picture with different weight tables unsupported" in capfd.readouterr().err
    # a P picture's first slice, then a hand-written B slice header where its second slice should start (the refusal comes with the
    # header, before any macroblock): the stream has pic_order_cnt_type 0 with 8-bit counts and 8-bit frame_num, CAVLC, PPS 0
    nals = list(N.split_annexb(lib, synth_cases.write_stream(tmp_path, "--mbw 6 --mbh 4 --frames 4 --seed 78 --refs 2 --bframes 1 --slices 2", "r")))
    parser = Parser(quiet=True, lib=lib)
    slices = 0
    with pytest.raises(P264Error):
        for typ, idc, rbsp in nals:
            if typ in (1, 5):
                slices += 1
                if slices == 4:                                       # (IDR: 2 slices; P: its first slice went in, this is its second)
                    h = BitWriter()
                    h.ue(12); h.ue(6); h.ue(0); h.u(8, 1); h.u(8, 4); h.u(1, 1); h.u(1, 0); h.u(1, 0); h.u(1, 0); h.se(0); h.ue(0); h.se(0); h.se(0)
                    h.trailing()
                    typ, idc, rbsp = 1, 0, h.bytes()
            parser.feed(typ, idc, rbsp)
    assert slices == 4
    assert "P and B slices in one picture unsupported" in capfd.readouterr().err


def test_offsets_outside_the_standards_range_are_refused(lib, capfd):
    """slice_alpha_c0_offset_div2 / slice_beta_offset_div2 beyond -6 .. 6 (7.4.3): a hand-written IDR slice header"""
    def sps_pps():
        s = BitWriter()
        s.u(8, 66); s.u(8, 0xc0); s.u(8, 40); s.ue(0); s.ue(0); s.ue(2); s.ue(1); s.u(1, 0); s.ue(0); s.ue(0); s.u(1, 1); s.u(1, 1); s.u(1, 0); s.u(1, 0); s.trailing()
        q = BitWriter()
        q.ue(0); q.ue(0); q.u(1, 0); q.u(1, 0); q.ue(0); q.ue(0); q.ue(0); q.u(1, 0); q.u(2, 0); q.se(0); q.se(0); q.se(0); q.u(1, 1); q.u(1, 0); q.u(1, 0); q.trailing()
        return s.bytes(), q.bytes()
    for alpha, beta, ok in ((6, -6, True), (7, 0, False), (0, -7, False)):
        p = Parser(quiet=True, lib=lib)
        sps, pps = sps_pps()
        p.feed(7, 3, sps); p.feed(8, 3, pps)
        h = BitWriter()
        h.ue(0); h.ue(7); h.ue(0); h.u(4, 0); h.ue(0); h.u(1, 0); h.u(1, 0); h.se(0); h.ue(0); h.se(alpha); h.se(beta)
        h.ue(3); h.u(1, 1)                                            # (an Intra16x16 macroblock type, then nothing: the data runs out)
        h.trailing()
        capfd.readouterr()
        try:
            p.feed(5, 3, h.bytes())
        except P264Error:
            pass
        err = capfd.readouterr().err
        assert ("out of range (-6 .. 6)" in err) == (not ok), (alpha, beta, err)


def test_a_sub_mb_type_past_the_int_range_is_refused(lib, tmp_path, capfd):
    """found by tests/tools/asan_slices.sh on a damaged stream: ue(v) codes of 32 zeros read as 0xffffffff, -1 as an int, and the
    sub_mb_type checks only looked at the upper end (the B path then indexed its tables at -1).  A hand-written P slice of a 1 x 1
    stream: header, mb_skip_run 0, mb_type P_8x8, then five zero bytes where the sub_mb_types should be."""
    nals = list(N.split_annexb(lib, synth_cases.write_stream(tmp_path, "--mbw 1 --mbh 1 --frames 2 --gop 0 --seed 3", "t")))
    assert [t for t, _, _ in nals] == [7, 8, 5, 1]
    parser = Parser(quiet=True, lib=lib)
    for typ, idc, rbsp in nals[:3]:
        parser.feed(typ, idc, rbsp)
    h = BitWriter()
    h.ue(0); h.ue(5); h.ue(0); h.u(8, 1); h.u(1, 0); h.u(1, 0); h.u(1, 0); h.se(0); h.ue(0); h.se(0); h.se(0)     # the P slice header
    h.ue(0); h.ue(3)                                                  # mb_skip_run 0, mb_type 3 = P_8x8
    h.u(8, 0); h.u(8, 0); h.u(8, 0); h.u(8, 0); h.u(8, 0); h.u(8, 0)
    h.trailing()
    capfd.readouterr()
    with pytest.raises(P264Error):
        parser.feed(1, 3, h.bytes())
    assert "invalid i_sub_partition" in capfd.readouterr().err


# ---- the records of parsed pictures through the packed and compact forms -----------------------------------------------------------
def test_parsed_pictures_with_deltas_through_the_compact_form(lib, tmp_path):
    """expand(pack_compact(p)) == pack_input(p) section by section and p264hip_compact_check passes - parsed pictures whose records
    carry deltas, I_PCM macroblocks among them"""
    pcm_with_deltas = with_deltas = 0
    for name in ("ipcm_p_cavlc", "b_cabac_temporal_3"):
        data, _ = ss.make(tmp_path, ss.STREAMS[name])
        for p in ss.parse(lib, data)[1]:
            rec = p.mb_records()
            packed = HipReconstructor.pack(p, lib)
            compact = HipReconstructor.pack_compact(p, lib)
            assert lib.p264hip_compact_check(C.byref(p.desc), compact.ctypes.data, compact.size) == 0
            back = HipReconstructor.expand_compact(p, compact, lib)
            lay = N.InputLayout()
            assert lib.p264hip_input_layout(C.byref(p.desc), C.byref(lay)) == 0
            n = p.n_mb
            sizes = {lay.off_mb: 16 * n, lay.off_mv: 64 * n, lay.off_ref: 4 * n, lay.off_i4: 16 * n, lay.off_coef: 32 * int(p.desc.n_coef_blocks)}
            if p.desc.slice_type == N.SLICE_B:
                sizes.update({lay.off_mv_l1: 64 * n, lay.off_ref_l1: 4 * n, lay.off_weights: 512})
            for off, size in sizes.items():
                assert np.array_equal(packed[off:off + size], back[off:off + size]), (name, off)
            assert np.array_equal(packed[lay.off_mb:lay.off_mb + 16 * n], p.mb)
            with_deltas += bool(rec["flags"].any())
            pcm_with_deltas += int(((rec["mb_type"] == N.MB_IPCM) & (rec["flags"] != 0)).sum())
    assert with_deltas >= 8 and pcm_with_deltas >= 5, (with_deltas, pcm_with_deltas)
