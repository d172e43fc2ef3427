"""constrained_intra_pred_flag (H.264 7.4.2.2; 8.3.1.1, 8.3.1.2, 8.3.3, 8.3.4; the reference reads the flag and drops it,
decoder/set.c:241) on the CPU side: the parser's `avail` and Intra4x4 modes against the stream writer's record
(synth264 --constrained-intra --dump-avail), its vectors against the writer's (the flag does not reach vector prediction), CAVLC
form = CABAC form, an all-intra stream that the flag leaves alone, streams without the option that stay what they were - and
the parsed pictures through the oracle and through tests/intra_checker.py.  Writer and parser share one author's reading of the
flag; what the intra predictors do with the availability it produces is checked by the intra checker, written from the
standard's text.  Every parser test fails on the parent, which left `avail` slice-shaped."""
import hashlib

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import synth_cases
from tests.hip_harness import decode_both
from tests.stream_args import CI, CI_STREAMS as STREAMS
from tests.synth_cases import write_stream as write

FIELDS = ("mb", "mv", "ref_idx", "i4modes", "coefs")


@pytest.mark.parametrize("cabac", [False, True], ids=["cavlc", "cabac"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_parser_against_the_writers_record(lib, tmp_path, name, cabac):
    args = STREAMS[name] + CI + (" --cabac" if cabac else "")
    data = write(tmp_path, args, dumps=("avail", "mv"))[0]
    pics = Parser(quiet=True, lib=lib).parse_stream(data)
    n = pics[0].n_mb
    dump = np.fromfile(str(tmp_path / "s.avail"), np.uint8).reshape(len(pics), n * 17)
    masked = i4 = 0
    for i, p in enumerate(pics):
        r = p.mb_records()
        assert np.array_equal(r["avail"], dump[i, :n]), "picture %d: avail" % i
        is4 = r["mb_type"] == N.MB_I4x4
        assert np.array_equal(p.i4modes.reshape(n, 16)[is4], dump[i, n:].reshape(n, 16)[is4]), "picture %d: Intra4x4 modes" % i
        if p.desc.slice_type != N.SLICE_I:
            i4 += int(is4.sum())
            # an intra macroblock next to an inter one: its flag towards that neighbour is off although the slice has it
            w = p.mb_w
            intra = r["mb_type"] <= N.MB_IPCM
            for m in np.flatnonzero(intra):
                m = int(m)
                if m % w and not intra[m - 1]:
                    assert not r["avail"][m] & N.AVAIL_LEFT
                    masked += 1
                if m >= w and not intra[m - w]:
                    assert not r["avail"][m] & N.AVAIL_TOP
    assert masked > 20 and i4 > 10, (masked, i4)


def test_vector_prediction_keeps_the_slices_availability(lib, tmp_path):
    """the writer predicts vectors from every neighbour of the slice, intra ones counting as 'intra' (8.4.1.3), whatever the
    flag says: the parser's vectors are the writer's"""
    data = write(tmp_path, STREAMS["sub8x8"] + CI, dumps=("avail", "mv"))[0]
    pics = Parser(quiet=True, lib=lib).parse_stream(data)
    n = pics[0].n_mb
    dump = np.fromfile(str(tmp_path / "s.mv"), np.uint8).reshape(len(pics), n * 64 + n * 16)
    inter_next_to_intra = 0
    for i, p in enumerate(pics):
        mv = dump[i, :n * 64].view(np.int16).reshape(n, 16, 2)
        inter = p.mb_records()["mb_type"] > N.MB_IPCM
        assert np.array_equal(p.mv.reshape(n, 16, 2)[inter], mv[inter]), "picture %d: vectors" % i
        t = inter.reshape(p.mb_h, p.mb_w)
        inter_next_to_intra += int((t[:, 1:] & ~t[:, :-1]).sum() + (t[1:] & ~t[:-1]).sum())
    assert inter_next_to_intra > 30


@pytest.mark.parametrize("name", list(STREAMS))
def test_cavlc_and_cabac_forms_parse_to_the_same_pictures(lib, tmp_path, name):
    args = STREAMS[name] + CI
    a = Parser(quiet=True, strict=True, lib=lib).parse_stream(write(tmp_path, args, "cavlc"))
    c = Parser(quiet=True, lib=lib).parse_stream(write(tmp_path, args + " --cabac", "cabac"))
    assert len(a) == len(c) == int(args.split("--frames ")[1].split()[0])
    for i, (p, q) in enumerate(zip(a, c)):
        assert p.desc.slice_type == q.desc.slice_type and p.desc.n_coef_blocks == q.desc.n_coef_blocks
        for f in FIELDS:
            assert np.array_equal(getattr(p, f), getattr(q, f)), "picture %d: %s differs" % (i, f)
        if p.desc.slice_type == N.SLICE_B:
            assert np.array_equal(p.mv_l1, q.mv_l1) and np.array_equal(p.ref_idx_l1, q.ref_idx_l1), "picture %d: list-1 motion differs" % i


def test_the_flag_changes_nothing_in_an_all_intra_stream(lib, tmp_path):
    args = "--mbw 9 --mbh 7 --frames 4 --intra-only --seed 406 --coded 30 --slices 2"
    plain, flagged = write(tmp_path, args, "a"), write(tmp_path, args + " --constrained-intra", "b")
    assert plain != flagged and len(plain) == len(flagged)
    diff = [i for i in range(len(plain)) if plain[i] != flagged[i]]
    pps = plain.index(b"\x00\x00\x00\x01\x68")
    assert len(diff) == 1 and pps < diff[0] < plain.index(b"\x00\x00\x00\x01", pps + 4), "more than one byte of the PPS differs"
    a, b = (Parser(quiet=True, lib=lib).parse_stream(s) for s in (plain, flagged))
    for p, q in zip(a, b):
        for f in FIELDS:
            assert np.array_equal(getattr(p, f), getattr(q, f)), f


@pytest.mark.parametrize("name", ["cif_ip", "qpd_dbo", "row_1xN", "mv_far"])
def test_streams_without_the_option_are_what_they_were(name):
    assert hashlib.sha256(synth_cases.stream_bytes(name)).hexdigest() == synth_cases.golden(name)[0]


def test_streams_of_other_features_without_the_option_are_what_they_were():
    name = "main_1080p_cabac_ipb"
    assert hashlib.sha256(open(synth_cases.generate(synth_cases.ORACLE_CASES[name]), "rb").read()).hexdigest() == synth_cases.oracle_golden(name)[0]


@pytest.mark.parametrize("name", list(STREAMS))
def test_oracle_equals_the_intra_checker_on_constrained_streams(oracle, lib, tmp_path, name):
    pics, n, first, chk = decode_both(oracle, lib, write(tmp_path, STREAMS[name] + CI + (" --cabac" if name in ("b", "ipcm") else "")))
    flags = {int(a) for p in pics if p.desc.slice_type != N.SLICE_I for a in p.mb_records()["avail"][p.mb_records()["mb_type"] <= N.MB_IPCM]}
    assert len(flags) >= 12, "only %d of the sixteen flag combinations on intra macroblocks of P / B pictures" % len(flags)
    assert n == 0, "%d samples differ, first: %s" % (n, first)
