"""Scaling matrices through the host parser, no GPU: hand-built SPS / PPS NALs put in front of a stream of the writer - fall-back rules
A and B for every list number, useDefaultScalingMatrixFlag, lists that end early, a PPS with and without transform_8x8_mode_flag, a
matrix in the SPS only, lists that spell out 16 - against tests/scaling_checker.py's reading of table 7-2; what stays refused
(without P264PARSE_OPT_SCALING everything, with it a second chroma offset that differs, other lists inside one picture, an
extension that ends inside its lists); the tail of a Main-profile PPS never fails; and the writer's own record (--dump-cqm) of the
streams the GPU tests decode."""
import os
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import scaling_checker as SC
from tests import scaling_stim as SS
from tests import synth_cases
from tests.test_t8x8_parser_cpu import Bits

GEOM = "--mbw 5 --mbh 4 --frames 3 --coded 40 --maxlevel 6 --qp 24 --refs 2"


def synth(tmp_path, args, dump=False):
    tool = synth_cases.ensure_tool()
    out, dmp = os.path.join(str(tmp_path), "s.264"), os.path.join(str(tmp_path), "s.cqm")
    subprocess.run([tool, out] + args.split() + (["--dump-cqm", dmp] if dump else []), check=True)
    return open(out, "rb").read(), (open(dmp, "rb").read() if dump else None)


def bits_of(rbsp):
    bits = [(byte >> (7 - i)) & 1 for byte in rbsp for i in range(8)]
    while not bits[-1]:
        bits.pop()
    return bits[:-1]                                                  # (without the stop bit)


def from_bits(bits):
    e = Bits()
    e.b = list(bits)
    return e


def put_lists(b, coded):
    """scaling_list_present_flag + scaling_list( ) per entry: None, "default" or the list"""
    for c in coded:
        if c is None:
            b.u(1, 0)
        elif isinstance(c, str):
            b.u(1, 1).se(-8)
        else:
            b.u(1, 1)
            for d in SC.deltas_of(c):
                b.se(d)
    return b


def read_ue(bits, at):
    z = 0
    while not bits[at + z]:
        z += 1
    v = int("".join(map(str, bits[at + z:at + 2 * z + 1])), 2) - 1
    return v, at + 2 * z + 1


class Carrier:
    """a stream of the writer whose parameter sets are rewritten: high = it was written with --t8x8 (its SPS has the High fields, its
    PPS the three-bit extension 1, 0, se(0) and its macroblocks carry transform_size_8x8_flag); else a Baseline stream whose SPS
    becomes a High one here and whose PPS gets an extension with transform_8x8_mode_flag 0"""

    def __init__(self, lib, tmp_path, args, high):
        self.lib, self.high = lib, high
        self.nals = list(N.split_annexb(lib, synth(tmp_path, GEOM + " " + args)[0]))
        assert self.nals[0][0] == 7 and self.nals[1][0] == 8

    def sps(self, coded=None):
        bits = bits_of(self.nals[0][2])
        if self.high:
            head, tail = bits[:31], bits[32:]                         # (profile, flags, level, ue(0), ue(1), ue(0), ue(0), bypass | matrices | ...)
        else:
            head, tail = [0, 1, 1, 0, 0, 1, 0, 0] + bits[8:25] + [0, 1, 0, 1, 1, 0], bits[25:]     # profile 100; chroma_format_idc 1, depths 8, no bypass
        b = from_bits(head).u(1, 0 if coded is None else 1)
        if coded is not None:
            put_lists(b, coded)
        b.b += tail
        return b.rbsp()

    def pps(self, coded=None, second=0, pps_id=0, cut=None):
        bits = bits_of(self.nals[1][2])
        if self.high:
            bits = bits[:-3]
        assert bits[0] == 1                                           # ue(0): the writer's pps id
        b = from_bits(Bits().ue(pps_id).b + bits[1:]).u(1, 1 if self.high else 0).u(1, 0 if coded is None else 1)
        if coded is not None:
            put_lists(b, coded[:8 if self.high else 6])
        b.se(second)
        if cut is not None:
            b.b = b.b[:len(b.b) - cut]
        return b.rbsp()

    def parse(self, sps, ppss, scaling=True, limit=None, slice_pps=None):
        """the pictures the parser hands out (refused NALs are skipped); slice_pps: {slice NAL number: pps id to write into its header}"""
        p = Parser(quiet=True, lib=self.lib, scaling=scaling)
        out, refused, n_slice = [], 0, 0
        feed = [(7, 3, sps)] + [(8, 3, q) for q in ppss] + self.nals[2:]
        for typ, idc, rbsp in feed:
            if typ in (1, 5):
                if slice_pps and n_slice in slice_pps:
                    bits = bits_of(rbsp)
                    _, at = read_ue(bits, 0)
                    _, at = read_ue(bits, at)
                    _, end = read_ue(bits, at)
                    rbsp = from_bits(bits[:at] + Bits().ue(slice_pps[n_slice]).b + bits[end:]).rbsp()
                n_slice += 1
            try:
                pic = p.feed(typ, idc, rbsp)
            except Exception:
                refused += 1
                continue
            if pic is not None:
                out.append(pic)
                if limit and len(out) >= limit:
                    break
        p.close()
        return out, refused


def table_of(pic):
    return bytes(pic.desc.scaling4x4) + bytes(pic.desc.scaling8x8)


@pytest.fixture(scope="module")
def high(lib, tmp_path_factory):
    return Carrier(lib, tmp_path_factory.mktemp("cqm_high"), "--seed 61 --t8x8 50", True)


@pytest.fixture(scope="module")
def plain(lib, tmp_path_factory):
    return Carrier(lib, tmp_path_factory.mktemp("cqm_plain"), "--seed 62", False)


def test_the_carriers_parse_as_they_are(high, plain):
    for c in (high, plain):
        pics, refused = c.parse(c.sps(), [c.pps()])
        assert len(pics) == 3 and not refused and not any(p.desc.scaling_lists for p in pics)
    assert all(p.desc.transform_8x8 for p in high.parse(high.sps(), [high.pps()])[0][1:])


def test_rules_a_and_b_for_every_list_number(high):
    r, q = SS.random_lists(50), SS.random_lists(51)
    seq_coded = [r[0], None, r[2], "default", r[4], None, None, r[7]]
    for n in range(8):
        alone = [None] * 8
        alone[n] = q[n]
        # rule A: in the SPS; in the PPS of a stream whose SPS has no matrix
        for sps, pps in ((alone, None), (None, alone)):
            pics, refused = high.parse(high.sps(sps), [high.pps(pps)], limit=1)
            assert not refused and pics[0].desc.scaling_lists == 1
            assert table_of(pics[0]) == SC.table_bytes(SC.resolve(alone)), (n, sps is None)
        # rule B: the PPS of a stream whose SPS has one
        pics, refused = high.parse(high.sps(seq_coded), [high.pps(alone)], limit=1)
        assert not refused and table_of(pics[0]) == SC.table_bytes(SC.resolve(alone, SC.resolve(seq_coded))), n
    # every list present at once, and none present at all (rule A: the defaults; rule B: the SPS's)
    assert table_of(high.parse(high.sps(q), [high.pps()], limit=1)[0][0]) == SC.table_bytes(q)
    assert table_of(high.parse(high.sps(), [high.pps([None] * 8)], limit=1)[0][0]) == SC.table_bytes(SC.DEFAULTS)
    assert table_of(high.parse(high.sps(seq_coded), [high.pps([None] * 8)], limit=1)[0][0]) == SC.table_bytes(SC.resolve([None] * 8, SC.resolve(seq_coded)))


def test_use_default_early_termination_and_a_matrix_in_the_sps_only(high):
    early = [list(x) for x in SS.random_lists(52)]
    for n, lst in enumerate(early):
        lst[len(lst) // 2:] = [lst[len(lst) // 2]] * (len(lst) - len(lst) // 2)
        assert len(SC.deltas_of(lst)) == len(lst) // 2 + 2
    coded = [early[0], "default", early[2], "default", early[4], early[5], "default", early[7]]
    want = SC.table_bytes(SC.resolve(coded))
    # in the SPS only: every picture takes the SPS's lists
    pics, refused = high.parse(high.sps(coded), [high.pps()])
    assert len(pics) == 3 and not refused and all(p.desc.scaling_lists == 1 and table_of(p) == want for p in pics)
    pics, _ = high.parse(high.sps(), [high.pps(coded)])
    assert len(pics) == 3 and all(table_of(p) == want for p in pics)


def test_a_pps_without_transform_8x8_mode_codes_six_lists(plain):
    q = SS.random_lists(53)
    coded = [q[0], None, "default", None, q[4], None]
    pics, refused = plain.parse(plain.sps(), [plain.pps(coded)])
    assert len(pics) == 3 and not refused
    assert all(table_of(p) == SC.table_bytes(SC.resolve(coded)) and p.desc.transform_8x8 == 0 for p in pics)      # 6, 7: the defaults (rule A)
    seq = [None, q[1], None, None, None, q[5], q[6], None]
    pics, refused = plain.parse(plain.sps(seq), [plain.pps(coded)])
    assert len(pics) == 3 and all(table_of(p) == SC.table_bytes(SC.resolve(coded, SC.resolve(seq))) for p in pics)
    assert table_of(pics[0])[96:160] == bytes(q[6])                                                              # 6: the SPS's (rule B)


def test_lists_that_spell_out_16_are_a_flat_picture(high):
    flat = SS.flat_lists()
    for sps, pps in ((flat, None), (None, flat), (SS.random_lists(54), flat)):
        pics, refused = high.parse(high.sps(sps), [high.pps(pps)])
        assert len(pics) == 3 and not refused
        assert all(p.desc.scaling_lists == 0 and table_of(p) == bytes(224) for p in pics)


def test_without_the_option_the_refusals_are_todays(high, capfd):
    q = SS.random_lists(55)
    pics, refused = high.parse(high.sps(q), [high.pps()], scaling=False)
    assert not pics and refused >= 4                                  # the SPS and, without one, every slice
    assert "flat lists" in capfd.readouterr().err
    pics, refused = high.parse(high.sps(), [high.pps(q)], scaling=False)
    assert not pics and refused == 3
    assert "pic_scaling_matrix_present_flag unsupported (flat scaling lists only)" in capfd.readouterr().err


def test_what_stays_refused_with_the_option(high, capfd):
    q = SS.random_lists(56)
    # a second chroma offset that differs from the first, now read behind the matrices too
    pics, refused = high.parse(high.sps(), [high.pps(q, second=2)])
    assert not pics and refused == 3 and "second_chroma_qp_index_offset 2 differs" in capfd.readouterr().err
    pics, refused = high.parse(high.sps(), [high.pps(None, second=-1)])
    assert not pics and "second_chroma_qp_index_offset -1 differs" in capfd.readouterr().err
    # an extension that ends inside its lists: refused when a slice of a High-profile SPS activates the set
    pics, refused = high.parse(high.sps(), [high.pps(q, cut=40)])
    assert not pics and refused == 3 and "ends inside the scaling matrix" in capfd.readouterr().err
    # an SPS that ends inside its lists: refused at once, no set
    sps = high.sps(q)
    pics, refused = high.parse(sps[:30], [high.pps()])
    assert not pics and refused >= 4


def test_the_tail_of_a_main_profile_pps_never_fails(lib, plain):
    """the PPS of a stream that is not High may end in anything: nothing of the tail is looked at"""
    want, _ = plain.parse(plain.nals[0][2], [plain.nals[1][2]])
    assert len(want) == 3
    q = SS.random_lists(57)
    for tail in (plain.pps(q), plain.pps(q, second=3), plain.pps(q, cut=40), plain.pps(q, cut=len(bits_of(plain.pps(q))) - len(bits_of(plain.nals[1][2])) - 2)):
        for scaling in (True, False):
            pics, refused = plain.parse(plain.nals[0][2], [tail], scaling=scaling)
            assert len(pics) == 3 and not refused
            for a, b in zip(want, pics):
                assert b.desc.scaling_lists == 0 and b.desc.transform_8x8 == 0
                for name in ("mb", "mv", "ref_idx", "i4modes", "coefs"):
                    assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_a_slice_with_other_lists_in_the_same_picture_is_refused(lib, tmp_path, capfd):
    c = Carrier(lib, tmp_path, "--seed 63 --slices 2", False)
    a, b = SS.random_lists(58)[:6], SS.random_lists(59)[:6]
    n_slices = sum(typ in (1, 5) for typ, _, _ in c.nals)
    assert n_slices == 6
    # the same lists through two PPSs: one picture
    pics, refused = c.parse(c.sps(), [c.pps(a), c.pps(a, pps_id=1)], slice_pps={1: 1})
    assert len(pics) == 3 and not refused and table_of(pics[0]) == SC.table_bytes(SC.resolve(a))
    capfd.readouterr()
    # other lists in the second slice of the first picture: the slice is refused, the picture never completes
    pics, refused = c.parse(c.sps(), [c.pps(a), c.pps(b, pps_id=1)], slice_pps={1: 1}, limit=1)
    assert refused >= 1 and "slices of one picture with different scaling lists unsupported" in capfd.readouterr().err
    assert not pics or table_of(pics[0]) != SC.table_bytes(SC.resolve(b))
    # flat in one slice, lists in the other
    pics, refused = c.parse(c.sps(), [c.pps(), c.pps(b, pps_id=1)], slice_pps={1: 1}, limit=1)
    assert refused >= 1 and "different scaling lists" in capfd.readouterr().err


STREAMS = {"jvt": "--cqm jvt --cqm-where sps", "rand": "--cqm rand:7 --cqm-where pps", "both": "--cqm rand:7 --cqm-where both", "jvt both": "--cqm jvt --cqm-where both",
           "jvt pps": "--cqm jvt --cqm-where pps", "rand sps": "--cqm rand:9 --cqm-where sps"}


@pytest.mark.parametrize("which", list(STREAMS))
def test_the_descriptors_table_is_the_writers(lib, tmp_path, which):
    args = GEOM + " --seed 64 --t8x8 60 --i8x8 40 --bframes 1 --cabac " + STREAMS[which]
    data, dump = synth(tmp_path, args, dump=True)
    pics = Parser(quiet=True, lib=lib, intra8x8=True, scaling=True).parse_stream(data)
    assert len(pics) == 3 and len(dump) == 3 * 224
    for i, p in enumerate(pics):
        assert p.desc.scaling_lists == 1 and table_of(p) == dump[224 * i:224 * i + 224], i
    if which.startswith("jvt"):
        assert dump[:224] == SC.table_bytes(SC.DEFAULTS)
    else:
        assert all(4 <= v <= 64 for v in dump) and len(set(dump[:224])) > 40
    if which == "both":
        other, _ = synth(tmp_path, args.replace("--cqm-where both", "--cqm-where sps"), dump=True)
        sps_only = table_of(Parser(quiet=True, lib=lib, intra8x8=True, scaling=True).parse_stream(other)[0])
        got = dump[:224]
        # lists 0, 3, 6: the SPS's (rule B); 1, 4, 7: the PPS's own; 2, 5: the list in front of them
        assert got[0:16] == sps_only[0:16] and got[48:64] == sps_only[48:64] and got[96:160] == sps_only[96:160]
        assert got[16:32] != sps_only[16:32] and got[32:48] == got[16:32] and got[64:80] != sps_only[64:80] and got[80:96] == got[64:80] and got[160:] != sps_only[160:]
    # the same stream without --cqm is the stream of before but for its parameter sets
    flat, _ = synth(tmp_path, args.replace(STREAMS[which], ""))
    a, b = list(N.split_annexb(lib, flat)), list(N.split_annexb(lib, data))
    assert len(a) == len(b) and all(x == y for x, y in zip(a[2:], b[2:])) and (a[0] != b[0] or a[1] != b[1])
    # and without the option the stream is refused as ever
    p = Parser(quiet=True, lib=lib, intra8x8=True)
    n = 0
    for typ, idc, rbsp in b:
        try:
            n += p.feed(typ, idc, rbsp) is not None
        except Exception:
            pass
    assert n == 0
