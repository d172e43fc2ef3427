"""second_chroma_qp_index_offset through the host parser, no GPU: streams whose PPS extension gives Cr an offset of its own
(synth264 --cqo2) parse under Parser(cr_offset=True) to pictures with chroma_qp_offset = the first offset and cr_qp_offset_delta =
second - first, and to the arrays of the same stream written without --cqo2; without the option every slice is refused with the
message it always was refused with; the delta's extremes; a Main-profile stream that carries the extension has delta 0."""
import numpy as np
import pytest

from p264decoder_amd import Parser
from p264decoder_amd import _native as N
from tests import cr_offset_stim as CS
from tests import synth_cases
from tests.test_t8x8_parser_cpu import with_pps_extension

ARRAYS = ("mb", "mv", "ref_idx", "i4modes", "coefs")
HIGH = dict(intra8x8=True, scaling=True)


def stream(args):
    return open(synth_cases.generate(args), "rb").read()


def feed_all(parser, lib, data):
    """(pictures, refused NAL units)"""
    pics, refused = [], 0
    for typ, idc, rbsp in N.split_annexb(lib, data):
        try:
            p = parser.feed(typ, idc, rbsp)
        except Exception:
            refused += 1
            continue
        if p is not None:
            pics.append(p)
    return pics, refused


@pytest.mark.parametrize("which", list(CS.STREAMS))
def test_the_delta_comes_out_and_nothing_else_changes(lib, which):
    data, twin = stream(CS.stream_args(which)), stream(CS.stream_args(which, cqo2=None))
    assert data != twin
    pics = Parser(quiet=True, lib=lib, cr_offset=True, **HIGH).parse_stream(data)
    same = Parser(quiet=True, lib=lib, cr_offset=True, **HIGH).parse_stream(twin)
    assert len(pics) == len(same) == 7
    types = {int(p.desc.slice_type) for p in pics}
    assert types == ({N.SLICE_I, N.SLICE_P, N.SLICE_B} if "--bframes" in CS.STREAMS[which] else {N.SLICE_I, N.SLICE_P})
    for a, b in zip(pics, same):
        assert (int(a.desc.chroma_qp_offset), int(a.desc.cr_qp_offset_delta)) == (3, -10)
        assert (int(b.desc.chroma_qp_offset), int(b.desc.cr_qp_offset_delta)) == (3, 0)
        assert int(a.desc.transform_8x8) == int(b.desc.transform_8x8) != 0
        for name in ARRAYS + (("mv_l1", "ref_idx_l1") if int(a.desc.slice_type) == N.SLICE_B else ()):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    # the stream without --cqo2 parses the same with the option off
    off = Parser(quiet=True, lib=lib, **HIGH).parse_stream(twin)
    assert len(off) == 7 and all(int(p.desc.cr_qp_offset_delta) == 0 for p in off)


@pytest.mark.parametrize("which", list(CS.STREAMS))
def test_without_the_option_every_slice_is_refused(lib, which, capfd):
    data = stream(CS.stream_args(which))
    pics, refused = feed_all(Parser(quiet=False, lib=lib, **HIGH), lib, data)
    assert pics == [] and refused == 7
    assert "second_chroma_qp_index_offset -7 differs from chroma_qp_index_offset 3: unsupported" in capfd.readouterr().err


@pytest.mark.parametrize("first,second", [(-12, 12), (12, -12), (0, 12), (-12, -11)])
def test_the_extremes_of_the_delta(lib, first, second):
    data = stream("--mbw 4 --mbh 3 --frames 3 --refs 2 --t8x8 40 --qp 20 --maxlevel 2 --seed 93 --cqo %d --cqo2 %d" % (first, second))
    pics = Parser(quiet=True, lib=lib, cr_offset=True, **HIGH).parse_stream(data)
    assert len(pics) == 3
    assert all((int(p.desc.chroma_qp_offset), int(p.desc.cr_qp_offset_delta)) == (first, second - first) for p in pics)


def test_cqo2_defaults_to_cqo_and_needs_the_extension():
    """every argument list of before writes the bytes of before: --cqo2 equal to --cqo is the stream without it, and without --t8x8
    (no PPS extension) the flag changes nothing"""
    high = "--mbw 4 --mbh 3 --frames 3 --refs 2 --t8x8 40 --seed 94 --cqo 5"
    assert stream(high) == stream(high + " --cqo2 5") != stream(high + " --cqo2 4")
    base = "--mbw 4 --mbh 3 --frames 3 --seed 95 --cqo -2"
    assert stream(base) == stream(base + " --cqo2 9")


@pytest.mark.parametrize("args", ["--refs 2 --seed 51", "--refs 2 --seed 52 --cabac --bframes 2"])
def test_a_main_profile_stream_that_carries_the_extension_has_delta_0(lib, args):
    """under any profile but High the extension is not looked at, option or not"""
    data = stream("--mbw 7 --mbh 5 --frames 7 " + args)
    plain = Parser(quiet=True, lib=lib).parse_stream(data)
    ext = Parser(quiet=True, lib=lib, cr_offset=True, **HIGH).parse_stream(with_pps_extension(lib, data, second_offset=5))
    assert len(ext) == len(plain) == 7
    for a, b in zip(plain, ext):
        assert int(b.desc.cr_qp_offset_delta) == 0 and int(b.desc.chroma_qp_offset) == int(a.desc.chroma_qp_offset)
        for name in ARRAYS:
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
