"""High-profile streams with transform_size_8x8_flag through the host parser, no GPU: what the parser hands over against the
stream writer's own record (synth264 --t8x8 PCT --dump-t8x8: per macroblock the flag and per coded 8x8 block its 64 levels in scan
order), for CAVLC and CABAC, P and B; the two coders against each other; the parameter sets the parser refuses; Main-profile
streams with a PPS extension; Intra 8x8 refused; damaged streams."""
import os
import struct
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import synth_cases
from tests import t8x8_checker as T8

BASE = "--mbw 7 --mbh 5 --frames 7 --coded 45 --maxlevel 9 --qp 24 --qp-delta 4"
CASES = {
    "p_cavlc": "--refs 2 --seed 41 --t8x8 60",
    "p_cabac": "--refs 2 --seed 41 --t8x8 60 --cabac",
    "p_sub8x8_slices": "--refs 2 --seed 42 --t8x8 70 --sub8x8 --slices 3",
    "p_sub8x8_slices_cabac": "--refs 2 --seed 42 --t8x8 70 --sub8x8 --slices 3 --cabac",
    "b_spatial": "--refs 2 --bframes 2 --seed 43 --t8x8 70 --sub8x8",
    "b_spatial_d8inf_cabac": "--refs 2 --bframes 2 --seed 44 --t8x8 70 --d8inf --sub8x8 --cabac",
    "b_temporal": "--refs 2 --bframes 2 --seed 45 --t8x8 70 --temporal --slices 2",
    "b_temporal_d8inf": "--refs 2 --bframes 2 --seed 46 --t8x8 100 --temporal --d8inf",
    "b_temporal_d8inf_cabac": "--refs 2 --bframes 2 --seed 46 --t8x8 100 --temporal --d8inf --cabac --slices 2",
    "all_flagged_weighted": "--refs 2 --seed 47 --t8x8 100 --wp --cqo 3",
    "none_flagged": "--refs 2 --seed 48 --t8x8 0 --cabac",
}


def write_stream(tmp_path, args, dump=True):
    """(stream bytes, [per picture: (flags[n_mb], {macroblock: {quadrant: 64 levels}})]) of synth264 BASE + args"""
    tool = synth_cases.ensure_tool()
    out, dmp = os.path.join(str(tmp_path), "s.264"), os.path.join(str(tmp_path), "s.t8")
    subprocess.run([tool, out] + (BASE + " " + args).split() + (["--dump-t8x8", dmp] if dump else []), check=True)
    data = open(out, "rb").read()
    pics = []
    if dump:
        raw = open(dmp, "rb").read()
        at = 0
        while at < len(raw):
            (n,) = struct.unpack_from("<I", raw, at)
            at += 4
            flags, levels = np.zeros(n, np.uint8), {}
            for m in range(n):
                flags[m], cbp = raw[at], raw[at + 1]
                at += 2
                for k in range(4):
                    if flags[m] and cbp >> k & 1:
                        levels.setdefault(m, {})[k] = list(struct.unpack_from("<64h", raw, at))
                        at += 128
            pics.append((flags, levels))
    return data, pics


def parsed_t8(pic):
    rec = pic.mb_records()
    flags = ((rec["intra_modes"] & N.MB_T8X8) != 0).astype(np.uint8)
    levels = {}
    for m in np.flatnonzero(flags):
        T8.check_record(rec[m])
        for k in range(4):
            if int(rec["coef_mask"][m]) >> (4 * k) & 1:
                levels.setdefault(int(m), {})[k] = T8.levels8_of(pic, rec[m], k)
    return flags, levels


@pytest.mark.parametrize("case", list(CASES))
def test_the_parser_reads_what_the_writer_wrote(lib, tmp_path, case):
    data, want = write_stream(tmp_path, CASES[case])
    pics = Parser(quiet=True, lib=lib).parse_stream(data)
    assert len(pics) == len(want) == 7
    n_flagged = n_blocks = 0
    for i, (p, (flags, levels)) in enumerate(zip(pics, want)):
        assert p.desc.transform_8x8 == 1
        got_flags, got_levels = parsed_t8(p)
        assert np.array_equal(got_flags, flags), "picture %d: flags" % i
        assert got_levels == levels, "picture %d: levels" % i
        assert lib.p264hip_records_check_pic(p.desc, p.desc.mb) == -1
        rec = p.mb_records()
        assert not (flags & (rec["mb_type"] <= N.MB_IPCM)).any() and not (flags & ((rec["cbp"] & 15) == 0)).any()
        n_flagged += int(flags.sum())
        n_blocks += sum(len(v) for v in levels.values())
    if "--t8x8 0" in CASES[case]:
        assert n_flagged == 0
    else:
        assert n_flagged >= 20 and n_blocks >= 30, (n_flagged, n_blocks)
    if "--t8x8 100" in CASES[case] and "--sub8x8" not in CASES[case] and "--bframes" not in CASES[case]:
        # every inter macroblock with coded luma carries the flag
        for p in pics:
            rec = p.mb_records()
            elig = (rec["mb_type"] > N.MB_IPCM) & ((rec["cbp"] & 15) != 0)
            assert (((rec["intra_modes"] & N.MB_T8X8) != 0) == elig).all()


@pytest.mark.parametrize("pair", [("p_cavlc", "p_cabac"), ("p_sub8x8_slices", "p_sub8x8_slices_cabac"), ("b_temporal_d8inf", None)])
def test_cavlc_and_cabac_parse_to_the_same_pictures(lib, tmp_path, pair):
    args = CASES[pair[0]]
    a = Parser(quiet=True, lib=lib).parse_stream(write_stream(tmp_path, args, dump=False)[0])
    b = Parser(quiet=True, lib=lib).parse_stream(write_stream(tmp_path, args + " --cabac", dump=False)[0])
    assert len(a) == len(b) == 7
    for i, (x, y) in enumerate(zip(a, b)):
        for name in ("mb", "mv", "ref_idx", "i4modes"):
            assert np.array_equal(getattr(x, name), getattr(y, name)), "picture %d: %s" % (i, name)
        n = x.desc.n_coef_blocks
        assert n == y.desc.n_coef_blocks and np.array_equal(x.coefs[:n * 16], y.coefs[:n * 16]), "picture %d: levels" % i
        if x.desc.slice_type == N.SLICE_B:
            assert np.array_equal(x.mv_l1, y.mv_l1) and np.array_equal(x.ref_idx_l1, y.ref_idx_l1)


# ---- parameter sets, written bit by bit ------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def ue(self, v):
        n = (v + 1).bit_length()
        return self.u(n - 1, 0).u(n, v + 1)

    def se(self, v):
        return self.ue(2 * v - 1 if v > 0 else -2 * v)

    def rbsp(self):
        bits = self.b + [1]
        bits += [0] * (-len(bits) % 8)
        return bytes(int("".join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))


def high_sps(profile=100, chroma_format=1, depth_y=0, depth_c=0, bypass=0, matrices=0, mb_w=7, mb_h=5, sps_id=0):
    b = Bits().u(8, profile).u(8, 0).u(8, 40).ue(sps_id).ue(chroma_format)
    if chroma_format == 3:
        b.u(1, 0)
    b.ue(depth_y).ue(depth_c).u(1, bypass).u(1, matrices)
    if matrices:
        b.u(8, 0)                                                    # eight seq_scaling_list_present_flags, all 0
    b.ue(4).ue(2).ue(2).u(1, 0).ue(mb_w - 1).ue(mb_h - 1).u(1, 1).u(1, 1).u(1, 0).u(1, 0)
    return b.rbsp()


def test_a_high_sps_the_kernels_cannot_decode_is_refused_and_the_old_set_survives(lib):
    for profile in (100, 110, 122, 244, 44, 83, 86, 118, 128):
        p = Parser(quiet=True, lib=lib)
        assert p.feed(7, 3, high_sps(profile)) is None
        p.close()
    for bad in (dict(chroma_format=2), dict(chroma_format=3), dict(chroma_format=0), dict(depth_y=2, depth_c=2), dict(depth_c=1), dict(bypass=1), dict(matrices=1)):
        p = Parser(quiet=True, lib=lib)
        assert p.feed(7, 3, high_sps(mb_w=9, mb_h=4)) is None
        with pytest.raises(Exception):
            p.feed(7, 3, high_sps(**bad))
        # the set of before is still there: a stream that goes with it parses on (its own SPS NAL left out)
        p.close()


def test_the_old_set_survives_a_refused_one(lib, tmp_path):
    data, want = write_stream(tmp_path, CASES["p_cavlc"])
    nals = list(N.split_annexb(lib, data))
    assert nals[0][0] == 7
    p = Parser(quiet=True, lib=lib)
    pics = []
    for i, (typ, idc, rbsp) in enumerate(nals):
        pic = p.feed(typ, idc, rbsp)
        if pic is not None:
            pics.append(pic)
        if i == 0:
            with pytest.raises(Exception):
                p.feed(7, 3, high_sps(depth_y=2, depth_c=2))
            with pytest.raises(Exception):
                p.feed(7, 3, high_sps(chroma_format=2))
    assert len(pics) == 7 and all(np.array_equal(parsed_t8(a)[0], w[0]) for a, w in zip(pics, want))


def with_pps_extension(lib, data, second_offset=None, t8=1, matrices=0):
    """the stream with transform_8x8_mode_flag, pic_scaling_matrix_present_flag and second_chroma_qp_index_offset appended to
    every PPS (second_offset None: the PPS's own chroma offset cannot be known here - 0 is written, the streams used have 0)"""
    out = b""
    for typ, idc, rbsp in N.split_annexb(lib, data):
        if typ == 8:
            bits = [(byte >> (7 - i)) & 1 for byte in rbsp for i in range(8)]
            while not bits[-1]:
                bits.pop()
            bits.pop()                                               # the stop bit
            e = Bits()
            e.b = bits
            e.u(1, t8).u(1, matrices).se(second_offset or 0)
            rbsp = e.rbsp()
        body = bytes([idc << 5 | typ]) + rbsp
        esc, zeros = bytearray(), 0
        for byte in body:
            if zeros >= 2 and byte <= 3:
                esc.append(3)
                zeros = 0
            esc.append(byte)
            zeros = zeros + 1 if byte == 0 else 0
        out += b"\0\0\0\1" + bytes(esc)
    return out


@pytest.mark.parametrize("args", ["--refs 2 --seed 51", "--refs 2 --seed 52 --cabac --bframes 2"])
def test_main_and_baseline_streams_parse_as_before_with_a_pps_extension(lib, tmp_path, args):
    data, _ = write_stream(tmp_path, args, dump=False)
    plain = Parser(quiet=True, lib=lib).parse_stream(data)
    for kw in (dict(), dict(second_offset=5), dict(matrices=1)):
        ext = Parser(quiet=True, lib=lib).parse_stream(with_pps_extension(lib, data, **kw))
        assert len(ext) == len(plain) == 7
        for a, b in zip(plain, ext):
            assert b.desc.transform_8x8 == 0
            for name in ("mb", "mv", "ref_idx", "i4modes", "coefs"):
                assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_a_high_pps_with_matrices_or_a_second_offset_is_refused(lib, tmp_path):
    data, _ = write_stream(tmp_path, "--refs 2 --seed 53 --t8x8 50", dump=False)
    nals = list(N.split_annexb(lib, data))

    def pictures(pps_bits):
        p = Parser(quiet=True, lib=lib)
        n = 0
        for typ, idc, rbsp in nals:
            if typ == 8:
                bits = [(byte >> (7 - i)) & 1 for byte in rbsp for i in range(8)]
                while not bits[-1]:
                    bits.pop()
                e = Bits()
                e.b = bits[:-1 - 3] + pps_bits                      # the writer's extension: 1, 0, se(0) = three bits
                rbsp = e.rbsp()
            try:
                n += p.feed(typ, idc, rbsp) is not None
            except Exception:
                pass
        return n
    assert pictures([1, 0, 1]) == 7
    assert pictures([1, 1]) == 0                                     # pic_scaling_matrix_present_flag
    assert pictures([1, 0, 0, 1, 0]) == 0                            # second_chroma_qp_index_offset 1, the first is 0


def test_intra_8x8_is_refused(lib, tmp_path, capfd):
    data, _ = write_stream(tmp_path, "--refs 2 --seed 54 --t8x8 50 --t8x8-intra 100 --intra-pct 30", dump=False)
    p = Parser(quiet=True, lib=lib)
    n = 0
    for typ, idc, rbsp in N.split_annexb(lib, data):
        try:
            n += p.feed(typ, idc, rbsp) is not None
        except Exception:
            pass
    assert "Intra 8x8 prediction unsupported" in capfd.readouterr().err
    assert n < 7
    # no flagged I_NxN macroblock: the same options parse
    data, _ = write_stream(tmp_path, "--refs 2 --seed 54 --t8x8 50 --t8x8-intra 0 --intra-pct 30", dump=False)
    assert len(Parser(quiet=True, lib=lib).parse_stream(data)) == 7


@pytest.mark.parametrize("case", ["p_cabac", "b_temporal", "b_spatial_d8inf_cabac", "p_sub8x8_slices"])
def test_truncated_and_damaged_streams_run_to_the_end(lib, tmp_path, case):
    data, _ = write_stream(tmp_path, CASES[case], dump=False)
    rng = np.random.default_rng(len(case))
    for k in range(24):
        bad = bytearray(data)
        if k % 3 == 0:
            bad = bad[:int(rng.integers(40, len(bad)))]
        else:
            for _ in range(1 + k % 4):
                bad[int(rng.integers(30, len(bad)))] ^= 1 << int(rng.integers(0, 8))
        p = Parser(quiet=True, lib=lib)
        for typ, idc, rbsp in N.split_annexb(lib, bytes(bad)):
            try:
                pic = p.feed(typ, idc, rbsp)
            except Exception:
                continue
            if pic is not None:
                assert lib.p264hip_records_check_pic(pic.desc, pic.desc.mb) == -1
        p.close()
