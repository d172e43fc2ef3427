"""Explicit weighted prediction on the host (H.264 7.3.3.2 / 7.4.3.2): the parser's pred_weight_table against what the stream
writer meant (--dump-wp), the refusals, and the weight table's way through the slot layout and the compact link format."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, P264Error, Parser, _native as N
from tests import synth_cases
from tests.stream_args import WP_STREAMS as STREAMS

WP_REC = 3 + 2 * 16 * 3 * 2          # int16 per picture in the writer's --dump-wp record


def write_stream(tmp_path, args, name="s"):
    data, dump = synth_cases.write_stream(tmp_path, args, name, dumps=("wp",))
    return data, np.fromfile(dump, np.int16).reshape(-1, WP_REC)


def parsed_tables(lib, data):
    parser = Parser(quiet=True, lib=lib)
    try:
        pics = parser.parse_stream(data)
    finally:
        parser.close()
    return pics


def assert_tables_match(pics, recs):
    assert len(pics) == len(recs)
    for k, (p, r) in enumerate(zip(pics, recs)):
        d = p.desc
        assert d.explicit_wp == r[0], "picture %d" % k
        if not r[0]:
            continue
        assert [d.wp_log2_denom[0], d.wp_log2_denom[1]] == [r[1], r[2]], "picture %d" % k
        got = np.ctypeslib.as_array(d.wp)
        n0, n1 = d.n_ref, (d.n_ref_l1 if d.slice_type == N.SLICE_B else 0)
        want = r[3:].reshape(2, 16, 3, 2)
        got = got.reshape(2, 16, 3, 2)
        assert np.array_equal(got[0, :n0], want[0, :n0]), "picture %d list 0" % k
        assert np.array_equal(got[1, :n1], want[1, :n1]), "picture %d list 1" % k
        assert d.weighted_bipred == 0


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_parser_reads_the_writers_tables(lib, tmp_path, name):
    data, recs = write_stream(tmp_path, STREAMS[name])
    pics = parsed_tables(lib, data)
    assert_tables_match(pics, recs)
    assert sum(int(r[0]) for r in recs) >= 3                    # the streams do carry tables


def test_duplicated_reference_has_two_weights(lib, tmp_path):
    data, recs = write_stream(tmp_path, STREAMS["dup"])
    pics = parsed_tables(lib, data)
    dup = [p for p in pics if p.desc.explicit_wp and p.desc.n_ref >= 2]
    assert dup
    for p in dup:
        d = p.desc
        assert d.ref_slot[0] == d.ref_slot[1]                   # one frame at indices 0 and 1 (8.2.4.3 reordering)
        w = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2)
        assert not np.array_equal(w[0, 0, 0], w[0, 1, 0])       # ... with different luma weights


def test_defaults_filled_in(lib, tmp_path):
    """references without coded weights: 2^denom, offset 0 (7.4.3.2)"""
    data, recs = write_stream(tmp_path, STREAMS["p_cavlc"])
    pics = parsed_tables(lib, data)
    seen = 0
    for p in pics:
        d = p.desc
        if not d.explicit_wp:
            continue
        w = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2)
        for i in range(d.n_ref):
            for c in range(3):
                if w[0, i, c, 0] == 1 << d.wp_log2_denom[min(c, 1)] and w[0, i, c, 1] == 0:
                    seen += 1
    assert seen > 0


def test_identity_tables_leave_the_macroblocks_alone(lib, tmp_path):
    base = "--mbw 6 --mbh 4 --frames 5 --gop 0 --seed 76 --refs 2 --sub8x8 --coded 20 --maxlevel 8"
    plain = parsed_tables(lib, write_stream(tmp_path, base, "a")[0])
    ident = parsed_tables(lib, write_stream(tmp_path, base + " --wp --wp-identity", "b")[0])
    assert len(plain) == len(ident)
    for a, b in zip(plain, ident):
        assert np.array_equal(a.mv, b.mv) and np.array_equal(a.ref_idx, b.ref_idx) and np.array_equal(a.coefs, b.coefs)
        assert a.desc.explicit_wp == 0
        assert b.desc.explicit_wp == (b.desc.slice_type == N.SLICE_P)


def test_slices_with_different_tables_are_refused(lib, tmp_path, capfd):
    data, _ = write_stream(tmp_path, "--mbw 6 --mbh 4 --frames 3 --gop 0 --seed 77 --wp --slices 2 --wp-slice-differ")
    with pytest.raises(P264Error):
        parsed_tables(lib, data)
    assert "different weight tables" in capfd.readouterr().err


def test_writer_without_the_options_is_unchanged(tmp_path):
    """the committed stream hashes depend on it: the new options draw no random numbers unless asked for"""
    import hashlib
    for name in ("cif_ip", "tiny_1x1", "qpdelta"):
        args = synth_cases.CASES[name][0]
        golden = open(os.path.join(synth_cases.GOLDEN, "synth_%s.sha256" % name)).read().split()[0]
        assert hashlib.sha256(synth_cases.write_stream(tmp_path, args, "u")).hexdigest() == golden


# ---- the table through the ABI --------------------------------------------------------------------------------------------
def weighted_picture(lib, tmp_path):
    data, _ = write_stream(tmp_path, STREAMS["b_cabac"])
    pics = parsed_tables(lib, data)
    return [p for p in pics if p.desc.explicit_wp and p.desc.slice_type == N.SLICE_B][0], [p for p in pics if p.desc.explicit_wp and p.desc.slice_type == N.SLICE_P][0]


def layout(lib, desc):
    lay = N.InputLayout()
    assert lib.p264hip_input_layout(C.byref(desc), C.byref(lay)) == 0
    return lay


def test_layout_adds_the_section_only_to_weighted_pictures(lib, tmp_path):
    for pic in weighted_picture(lib, tmp_path):
        lw = layout(lib, pic.desc)
        d = N.Picture()
        C.memmove(C.byref(d), C.byref(pic.desc), C.sizeof(N.Picture))
        d.explicit_wp = 0
        lu = layout(lib, d)
        assert lu.off_wp == 0 and lw.off_wp == lu.bytes and lw.bytes == lu.bytes + 512
        for f in ("off_mb", "off_mv", "off_ref", "off_i4", "off_coef", "off_mv_l1", "off_ref_l1", "off_weights"):
            assert getattr(lw, f) == getattr(lu, f)


def test_pack_and_compact_round_trip_the_table(lib, tmp_path):
    for pic in weighted_picture(lib, tmp_path):
        packed = HipReconstructor.pack(pic, lib)
        lay = layout(lib, pic.desc)
        assert np.array_equal(packed[lay.off_wp:lay.off_wp + 384].view(np.int16), np.ctypeslib.as_array(pic.desc.wp))
        compact = HipReconstructor.pack_compact(pic, lib)
        hdr = N.CompactHdr.from_buffer_copy(compact[:C.sizeof(N.CompactHdr)].tobytes())
        assert hdr.off_wp and hdr.off_wp + 384 <= hdr.bytes
        assert lib.p264hip_compact_check(C.byref(pic.desc), compact.ctypes.data, compact.size) == 0
        back = HipReconstructor.expand_compact(pic, compact, lib)
        assert np.array_equal(back[lay.off_wp:lay.off_wp + 384], packed[lay.off_wp:lay.off_wp + 384])
        # unpack_input points back into the block; the descriptor keeps its table
        out = N.Picture()
        assert lib.p264hip_unpack_input(C.byref(pic.desc), packed.ctypes.data, C.c_size_t(packed.size), C.byref(out)) == 0
        assert out.explicit_wp == 1 and list(out.wp) == list(pic.desc.wp)


def test_unweighted_compact_bytes_unchanged(lib, f26):
    """an unweighted picture's compact block has no wp section (off_wp stays 0) - the header reads as it did"""
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(f26, limit=3)
    parser.close()
    for p in pics:
        compact = HipReconstructor.pack_compact(p, lib)
        hdr = N.CompactHdr.from_buffer_copy(compact[:C.sizeof(N.CompactHdr)].tobytes())
        assert hdr.off_wp == 0 and list(hdr.reserved) == [0] * 10
        assert layout(lib, p.desc).off_wp == 0


@pytest.mark.parametrize("field,value", [("denom", 8), ("denom", -1), ("weight", 129), ("weight", -129), ("offset", 128), ("offset", -129), ("implicit", 1)])
def test_out_of_range_tables_are_refused(lib, tmp_path, field, value):
    pic = weighted_picture(lib, tmp_path)[0]
    good = HipReconstructor.pack_compact(pic, lib)
    d = pic.desc
    keep = N.Picture()
    C.memmove(C.byref(keep), C.byref(d), C.sizeof(N.Picture))
    if field == "denom":
        d.wp_log2_denom[1] = value
    elif field == "weight":
        d.wp[6 * 1 + 2] = value                 # list 0, index 1, Cb weight
    elif field == "offset":
        d.wp[6 * 16 + 1] = value                # list 1, index 0, luma offset
    else:
        d.weighted_bipred = value
    try:
        assert lib.p264hip_wp_check(C.byref(d)) != 0
        with pytest.raises(P264Error):
            HipReconstructor.pack(pic, lib)
        with pytest.raises(P264Error):
            HipReconstructor.pack_compact(pic, lib)
        if field in ("weight", "offset"):
            # the same value inside a compact block (a producer that packed it wrongly): the full check refuses it
            bad = good.copy()
            hdr = N.CompactHdr.from_buffer_copy(bad[:C.sizeof(N.CompactHdr)].tobytes())
            k = (6 * 1 + 2) if field == "weight" else (6 * 16 + 1)
            bad[hdr.off_wp:hdr.off_wp + 384].view(np.int16)[k] = value
            assert lib.p264hip_compact_check(C.byref(keep), bad.ctypes.data, bad.size) != 0
    finally:
        C.memmove(C.byref(d), C.byref(keep), C.sizeof(N.Picture))
    assert lib.p264hip_wp_check(C.byref(d)) == 0


def test_bipred_pairs_past_the_limit_are_refused(lib, tmp_path, capfd):
    """8.4.2.3: a bi-predicted block whose two luma weights add up past 128 (the writer puts 100 on every entry)"""
    data, _ = write_stream(tmp_path, "--mbw 5 --mbh 4 --frames 5 --seed 78 --refs 2 --bframes 2 --wp --wp-bi --wp-bad-sum --coded 20 --maxlevel 8")
    with pytest.raises(P264Error):
        parsed_tables(lib, data)
    assert "add up to 200" in capfd.readouterr().err


def test_unpack_input_gives_the_blocks_table(lib, tmp_path):
    pic = weighted_picture(lib, tmp_path)[0]
    packed = HipReconstructor.pack(pic, lib)
    lay = layout(lib, pic.desc)
    packed[lay.off_wp:lay.off_wp + 384].view(np.int16)[0] = 77
    out = N.Picture()
    assert lib.p264hip_unpack_input(C.byref(pic.desc), packed.ctypes.data, C.c_size_t(packed.size), C.byref(out)) == 0
    assert out.wp[0] == 77


def test_k_mc_wp_does_not_spill(lib):
    """the weighted instance of k_mc at three wavefronts per SIMD - no spills, no scratch"""
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:                         # no ROCm LLVM tools on this machine
        pytest.skip(str(e))
    r = res["k_mc_wp"]
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0
    assert r["vgpr_count"] <= 168                    # three wavefronts per SIMD (512 / 3, in granules of 8)
    for k in ("k_mc_sort_wp", "k_mc_sort_b_wp"):     # the sort's instances for weighted batches
        assert res[k]["vgpr_spill_count"] == 0 and res[k]["private_segment_fixed_size"] == 0, k


@pytest.mark.parametrize("args", [
    "--mbw 8 --mbh 6 --frames 6 --gop 0 --seed 91 --refs 3 --mmco --sub8x8 --slices 2 --coded 25 --maxlevel 8 --wp --wp-identity",
    "--mbw 7 --mbh 5 --frames 8 --seed 92 --refs 2 --bframes 2 --cabac --coded 25 --maxlevel 8 --wp --wp-bi --wp-identity",
])
def test_checker_with_identity_weights_is_the_oracle(lib, oracle, tmp_path, args):
    """the weighted-prediction checker (tests/wp_checker.py) against oracle_reconstruct: with weight 2^denom and offset 0 the two
    are the same decoder, bit for bit, loop filter on"""
    from tests import oracle_bind, wp_checker
    data, _ = write_stream(tmp_path, args)
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    slots = parser.slots
    parser.close()
    assert sum(p.desc.explicit_wp for p in pics) >= 3
    chk = wp_checker.WeightedChecker(oracle, pics[0].mb_w, pics[0].mb_h, slots)
    ref = oracle_bind.FrameStore(pics[0].mb_w, pics[0].mb_h, slots)
    for k, p in enumerate(pics):
        got = chk.reconstruct(p)
        want = oracle_bind.reconstruct(oracle, ref, p)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "picture %d plane %d" % (k, c)


def clip1(x):
    return 0 if x < 0 else 255 if x > 255 else x


def weighted_sample(p0, p1, w0, o0, w1, o1, log_wd, pred_l0, pred_l1):
    """H.264 8.4.2.3.2 on Python integers, as the text states it (>> on a negative value rounds towards minus infinity, as in the
    standard's arithmetic): one list - Clip1(((predPartLX * wX + 2^(logWD - 1)) >> logWD) + oX) for logWD >= 1, else
    Clip1(predPartLX * wX + oX); both lists - Clip1(((predPartL0 * w0 + predPartL1 * w1 + 2^logWD) >> (logWD + 1)) + ((o0 + o1 + 1) >> 1))"""
    if pred_l0 and pred_l1:
        return clip1(((p0 * w0 + p1 * w1 + 2 ** log_wd) >> (log_wd + 1)) + ((o0 + o1 + 1) >> 1))
    p, w, o = (p0, w0, o0) if pred_l0 else (p1, w1, o1)
    if log_wd >= 1:
        return clip1(((p * w + 2 ** (log_wd - 1)) >> log_wd) + o)
    return clip1(p * w + o)


def test_both_weighting_helpers_follow_the_standard():
    """wp_checker._weigh and test_gpu_weighted_pred.weigh (the two numpy versions the GPU tests trust) against weighted_sample:
    every logWD, the ends of the weight and offset ranges, the inferred 2^logWD and 128, weight sums past the 8.4.2.3 limit, and
    samples at 0, 1, 127, 128, 254, 255 in both lists"""
    from tests import test_gpu_weighted_pred, wp_checker
    samples = [0, 1, 127, 128, 254, 255]
    p0 = np.array([a for a in samples for _ in samples], np.int64).reshape(6, 6)
    p1 = np.array([b for _ in samples for b in samples], np.int64).reshape(6, 6)
    offsets = [-128, -1, 0, 1, 127]
    past = 0
    for d in range(8):
        weights = sorted({-128, -127, -1, 0, 1, 1 << d, 127, 128})
        for w0, o0 in itertools.product(weights, offsets):
            # (one list: the other list's entry is another (weight, offset) - a helper that takes the wrong list's pair fails)
            w1, o1 = (-w0 - 1 if w0 < 128 else -128), -o0 - 1
            for l0, l1 in ((True, False), (False, True)):
                want = np.array([[weighted_sample(int(a), int(b), w0, o0, w1, o1, d, l0, l1) for a, b in zip(ra, rb)] for ra, rb in zip(p0, p1)])
                got = wp_checker._weigh(p0 if l0 else None, p1 if l1 else None, l0, l1, (w0, o0), (w1, o1), d)
                assert np.array_equal(got, want), (d, w0, o0, l0)
                assert np.array_equal(test_gpu_weighted_pred.weigh(p0, p1, l0, l1, (w0, o0), (w1, o1), d), want), (d, w0, o0, l0)
            for w1, o1 in itertools.product(weights, offsets[::2]):
                past += not -128 <= w0 + w1 <= (127 if d == 7 else 128)
                want = np.array([[weighted_sample(int(a), int(b), w0, o0, w1, o1, d, True, True) for a, b in zip(ra, rb)] for ra, rb in zip(p0, p1)])
                assert np.array_equal(wp_checker._weigh(p0, p1, True, True, (w0, o0), (w1, o1), d), want), (d, w0, o0, w1, o1)
                assert np.array_equal(test_gpu_weighted_pred.weigh(p0, p1, True, True, (w0, o0), (w1, o1), d), want), (d, w0, o0, w1, o1)
    assert past > 100


@pytest.mark.parametrize("mode", ["legal", "wide"])
def test_seam_fuzz_weight_tables(lib, mode):
    """tests/seam_fuzz.draw_wp_table: tables p264hip_wp_check accepts, forced denominators kept, Cb and Cr of an entry never one
    table, the 8.4.2.3 limit kept ("legal") or broken ("wide") on the pairs bi-predicted blocks use, both ends of the ranges drawn"""
    from tests import seam_fuzz
    rng = np.random.default_rng(5 if mode == "legal" else 6)
    ends, broken = set(), 0
    for i in range(12):
        den = (i % 8, 7 - i % 8)
        pic = seam_fuzz.make_picture(rng, 6, 4, n_ref=3, n_ref_l1=3, slots=4, b_picture=i % 3 != 0, explicit_wp=mode, wp_denoms=den,
                                     dup_refs=i % 2 == 1, past_list=0.2)
        d = pic.desc
        assert lib.p264hip_wp_check(C.byref(d)) == 0 and d.explicit_wp == 1 and d.weighted_bipred == 0
        assert (d.wp_log2_denom[0], d.wp_log2_denom[1]) == den
        t = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2).astype(int)
        assert all(tuple(t[l, k, 1]) != tuple(t[l, k, 2]) for l in range(2) for k in range(16))
        ends |= {int(w) for w in t[..., 0].reshape(-1) if abs(w) >= 127} | {("o", int(o)) for o in t[..., 1].reshape(-1) if o in (-128, 127)}
        for a, b in seam_fuzz.bi_pairs(pic):
            for c in range(3):
                broken += not seam_fuzz.wp_limit_ok(int(t[0, a, c, 0]), int(t[1, b, c, 0]), den[min(c, 1)])
        if i % 2 == 1:
            assert d.ref_slot[0] == d.ref_slot[1] and not np.array_equal(t[0, 0], t[0, 1])
    assert ends >= {-128, 127, 128, ("o", -128), ("o", 127)}, ends
    assert (broken == 0) if mode == "legal" else (broken > 10), broken


@pytest.mark.parametrize("b_picture", [False, True])
def test_checker_with_identity_weights_is_the_oracle_on_seam_pictures(lib, oracle, b_picture):
    """as test_checker_with_identity_weights_is_the_oracle, on seam-fuzz pictures no stream carries: intra macroblocks, three
    slices with deblocking idc 2, 0 and 1, sub-4x4 partitions, int16-wrapping levels and indices past their list - steps 2 and 3
    of the checker (the oracle's residual after a prediction from S, its loop filter with the picture's own motion) proven on them.
    The oracle gets the indices as drawn: past the list it predicts and filters from entry 0 like the checker."""
    from tests import oracle_bind, seam_fuzz, wp_checker
    rng = np.random.default_rng(31 + b_picture)
    mb_w, mb_h, slots = 7, 5, 5
    chk = wp_checker.WeightedChecker(oracle, mb_w, mb_h, slots)
    ref = oracle_bind.FrameStore(mb_w, mb_h, slots)
    for s in range(slots):
        f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth")
        for a, b, src in zip(chk.store[s], ref[s], f):
            a[:] = src
            b[:] = src
    past = 0
    for i in range(6):
        pic = seam_fuzz.make_picture(rng, mb_w, mb_h, p_picture=i != 2, dst_slot=i % slots, n_ref=3, n_ref_l1=2, slots=slots, b_picture=b_picture,
                                     level_style="mixed", qp_mode="random", intra_share=0.3, slices=3, slice_idcs=[2, 0, 1], mv_range=20,
                                     explicit_wp="wide", past_list=0.25)
        d = pic.desc
        if d.slice_type != N.SLICE_I:
            t = np.ctypeslib.as_array(d.wp).reshape(2, 16, 3, 2)
            for c in range(3):
                t[:, :, c] = (1 << d.wp_log2_denom[min(c, 1)], 0)
        past += int((pic.ref_idx >= d.n_ref).sum())
        plain = wp_checker._Copy(pic)
        plain.desc.explicit_wp = 0
        got = chk.reconstruct(pic)
        oracle.oracle_reconstruct(C.byref(plain.desc), ref.ptrs)
        want = ref[d.dst_slot]
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "picture %d plane %d" % (i, c)
    assert past > 20
