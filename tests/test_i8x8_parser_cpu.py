"""The host parser on Intra 8x8 macroblocks (P264PARSE_OPT_INTRA8X8; H.264 7.3.5, 7.3.5.1, 8.3.2.1): what it hands over against the
stream writer's own records (synth264 --t8x8 PCT --i8x8 PCT, --dump-i8x8: per macroblock the flag and the four modes; --dump-t8x8:
the flag, the coded 8x8 blocks and their 64 levels in scan order), CAVLC and CABAC, I / P / B slices, several slices, constrained
intra prediction; without the option the message of always; one I slice assembled bit by bit, which shares nobody's reading of the
syntax with the writer; damaged streams."""
import os
import struct
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import i8x8_checker as I8
from tests import synth_cases
from tests import t8x8_checker as T8

BASE = "--mbw 7 --mbh 5 --frames 7 --coded 45 --maxlevel 9 --qp 24 --qp-delta 4 --intra-pct 30"
CASES = {
    "p_cavlc": "--refs 2 --seed 61 --t8x8 60 --i8x8 60",
    "p_cabac": "--refs 2 --seed 61 --t8x8 60 --i8x8 60 --cabac",
    "p_two_slices": "--refs 2 --seed 62 --t8x8 50 --i8x8 70 --slices 2",
    "p_two_slices_cabac": "--refs 2 --seed 62 --t8x8 50 --i8x8 70 --slices 2 --cabac",
    "b_cavlc": "--refs 2 --bframes 2 --seed 63 --t8x8 60 --i8x8 60 --d8inf",
    "b_cabac_two_slices": "--refs 2 --bframes 2 --seed 64 --t8x8 60 --i8x8 60 --d8inf --cabac --slices 2",
    "constrained_intra": "--refs 2 --seed 65 --t8x8 60 --i8x8 60 --constrained-intra",
    "constrained_intra_b_cabac": "--refs 2 --bframes 2 --seed 66 --t8x8 60 --i8x8 60 --constrained-intra --cabac --slices 2",
    "all_flagged_with_ipcm": "--refs 2 --seed 67 --t8x8 100 --i8x8 100 --ipcm 10 --cabac",
    "none_flagged": "--refs 2 --seed 68 --t8x8 50 --i8x8 0",
}


def write_stream(tmp_path, args, dump=True):
    """(stream bytes, [per picture: (flag and modes uint8[n_mb][5], any-8x8 flags[n_mb], {macroblock: {quadrant: 64 levels}})])"""
    tool = synth_cases.ensure_tool()
    out, d8, di = (os.path.join(str(tmp_path), n) for n in ("s.264", "s.t8", "s.i8"))
    subprocess.run([tool, out] + (BASE + " " + args).split() + (["--dump-t8x8", d8, "--dump-i8x8", di] if dump else []), check=True)
    data = open(out, "rb").read()
    pics = []
    if dump:
        raw, rawi = open(d8, "rb").read(), open(di, "rb").read()
        at = ati = 0
        while at < len(raw):
            (n,) = struct.unpack_from("<I", raw, at)
            assert struct.unpack_from("<I", rawi, ati) == (n,)
            modes = np.frombuffer(rawi, np.uint8, n * 5, ati + 4).reshape(n, 5)
            at, ati = at + 4, ati + 4 + 5 * n
            flags, levels = np.zeros(n, np.uint8), {}
            for m in range(n):
                flags[m], cbp = raw[at], raw[at + 1]
                at += 2
                for k in range(4):
                    if flags[m] and cbp >> k & 1:
                        levels.setdefault(m, {})[k] = list(struct.unpack_from("<64h", raw, at))
                        at += 128
            pics.append((modes, flags, levels))
        assert ati == len(rawi)
    return data, pics


def parsed_8x8(pic):
    """(Intra 8x8 flags, flags of either kind, {macroblock: {quadrant: 64 levels}}) of a parsed picture"""
    rec = pic.mb_records()
    i8 = (rec["intra_modes"] & N.MB_I8X8) != 0
    both = i8 | ((rec["intra_modes"] & N.MB_T8X8) != 0)
    levels = {}
    for m in np.flatnonzero(both):
        (I8 if i8[m] else T8).check_record(rec[m])
        for k in range(4):
            if int(rec["coef_mask"][m]) >> (4 * k) & 1:
                levels.setdefault(int(m), {})[k] = T8.levels8_of(pic, rec[m], k)
    return i8, both.astype(np.uint8), levels


@pytest.mark.parametrize("case", list(CASES))
def test_the_parser_reads_what_the_writer_wrote(lib, tmp_path, case):
    data, want = write_stream(tmp_path, CASES[case])
    pics = Parser(quiet=True, lib=lib, intra8x8=True).parse_stream(data)
    assert len(pics) == len(want) == 7
    n_i8 = n_blocks = 0
    types = set()
    for i, (p, (modes, flags, levels)) in enumerate(zip(pics, want)):
        i8, both, got_levels = parsed_8x8(p)
        rec = p.mb_records()
        assert np.array_equal(i8, modes[:, 0] != 0), "picture %d: Intra 8x8 flags" % i
        assert np.array_equal(both, flags), "picture %d: transform flags" % i
        assert got_levels == levels, "picture %d: levels" % i
        for m in np.flatnonzero(i8):
            assert p.i4modes[m * 16:m * 16 + 16].tolist() == np.repeat(modes[m, 1:], 4).tolist(), "picture %d macroblock %d: modes" % (i, m)
            assert rec["mb_type"][m] == N.MB_I4x4 and (int(rec["coef_mask"][m]) & 0xffff) == sum(0xF << (4 * k) for k in levels.get(int(m), {}))
            assert (int(rec["cbp"][m]) & 15) >= sum(1 << k for k in levels.get(int(m), {}))
            n_blocks += len(levels.get(int(m), {}))
        assert bool(p.desc.transform_8x8 & N.T8X8_INTRA) == bool(i8.any()) and p.desc.transform_8x8 & 1
        assert lib.p264hip_records_check_pic(p.desc, p.desc.mb) == -1
        n_i8 += int(i8.sum())
        types |= {int(p.desc.slice_type)} if i8.any() else set()
    if "--i8x8 0" in CASES[case]:
        assert n_i8 == 0
        return
    assert n_i8 >= 20 and n_blocks >= 20, (n_i8, n_blocks)
    assert types >= ({N.SLICE_I, N.SLICE_P, N.SLICE_B} if "--bframes" in CASES[case] else {N.SLICE_I, N.SLICE_P}), types
    if "--i8x8 100" in CASES[case]:
        for p in pics:
            rec = p.mb_records()
            assert (((rec["intra_modes"] & N.MB_I8X8) != 0) == (rec["mb_type"] == N.MB_I4x4)).all()
            assert (rec["mb_type"] == N.MB_IPCM).any() or p.desc.slice_type != N.SLICE_I


@pytest.mark.parametrize("pair", ["p_cavlc", "p_two_slices", "b_cavlc", "constrained_intra"])
def test_cavlc_and_cabac_parse_to_the_same_pictures(lib, tmp_path, pair):
    args = CASES[pair]
    a = Parser(quiet=True, lib=lib, intra8x8=True).parse_stream(write_stream(tmp_path, args, dump=False)[0])
    b = Parser(quiet=True, lib=lib, intra8x8=True).parse_stream(write_stream(tmp_path, args + " --cabac", dump=False)[0])
    assert len(a) == len(b) == 7
    for i, (x, y) in enumerate(zip(a, b)):
        for name in ("mb", "mv", "ref_idx", "i4modes"):
            assert np.array_equal(getattr(x, name), getattr(y, name)), "picture %d: %s" % (i, name)
        n = x.desc.n_coef_blocks
        assert n == y.desc.n_coef_blocks and np.array_equal(x.coefs[:n * 16], y.coefs[:n * 16]), "picture %d: levels" % i


def test_without_the_option_the_old_message(lib, tmp_path, capfd):
    data, _ = write_stream(tmp_path, CASES["p_cabac"], dump=False)
    p = Parser(quiet=True, lib=lib)
    n = 0
    for typ, idc, rbsp in N.split_annexb(lib, data):
        try:
            n += p.feed(typ, idc, rbsp) is not None
        except Exception:
            pass
    assert "Intra 8x8 prediction unsupported" in capfd.readouterr().err
    assert n < 7


def test_a_stream_without_intra_8x8_parses_the_same_with_and_without_the_option(lib, tmp_path):
    for args in ("--refs 2 --seed 69 --t8x8 60", "--refs 2 --bframes 2 --seed 70 --t8x8 60 --cabac --d8inf", "--refs 2 --seed 71"):
        data, _ = write_stream(tmp_path, args, dump=False)
        a = Parser(quiet=True, lib=lib).parse_stream(data)
        b = Parser(quiet=True, lib=lib, intra8x8=True).parse_stream(data)
        assert len(a) == len(b) == 7
        for x, y in zip(a, b):
            assert bytes(x.desc)[:N.Picture.mb.offset] == bytes(y.desc)[:N.Picture.mb.offset] and x.desc.transform_8x8 == y.desc.transform_8x8
            for name in ("mb", "mv", "ref_idx", "i4modes", "coefs"):
                assert np.array_equal(getattr(x, name), getattr(y, name)), name


# ---- one I slice, bit by bit ------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.b = []

    def u(self, n, v):
        self.b += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bits(self, s):
        self.b += [int(c) for c in s.replace(" ", "")]
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


def test_an_i_slice_assembled_by_hand(lib):
    """two macroblocks side by side, CAVLC, QP 26, loop filter off: an Intra 8x8 macroblock, then an Intra4x4 macroblock whose mode
    predictions come out of it (8.3.1.1: Intra8x8PredMode[luma4x4BlkIdxN >> 2])"""
    # SPS: High, 4:2:0, 8 bits, no matrices; log2_max_frame_num 8, POC type 2, 2 reference frames, 2 x 1 macroblocks, frame_mbs_only,
    # direct_8x8_inference, no cropping, no VUI
    sps = Bits().u(8, 100).u(8, 0).u(8, 40).ue(0).ue(1).ue(0).ue(0).u(1, 0).u(1, 0).ue(4).ue(2).ue(2).u(1, 0).ue(1).ue(0).u(1, 1).u(1, 1).u(1, 0).u(1, 0).rbsp()
    # PPS: CAVLC, one slice group, one reference per list, no weights, QP 26, chroma offset 0, deblocking_filter_control_present,
    # then transform_8x8_mode_flag 1, no matrices, second offset 0
    pps = Bits().ue(0).ue(0).u(1, 0).u(1, 0).ue(0).ue(0).ue(0).u(1, 0).u(2, 0).se(0).se(0).se(0).u(1, 1).u(1, 0).u(1, 0).u(1, 1).u(1, 0).se(0).rbsp()
    s = Bits()
    # slice header (IDR): first_mb 0, type 7 (I), PPS 0, frame_num 0 in 8 bits, idr_pic_id 0, no_output_of_prior_pics 0, long_term 0,
    # slice_qp_delta 0, disable_deblocking_filter_idc 1
    s.ue(0).ue(7).ue(0).u(8, 0).ue(0).u(1, 0).u(1, 0).se(0).ue(1)
    # ---- macroblock 0: I_NxN, transform_size_8x8_flag 1
    s.ue(0).u(1, 1)
    s.bits("1")            # block 0: no neighbour, predictor 2; prev flag 1 -> mode 2 (DC)
    s.bits("0 111")        # block 1: A = block 0 = 2, B missing -> predictor 2; rem 7 -> mode 8 (horizontal-up)
    s.bits("0 000")        # block 2: A missing -> predictor 2; rem 0 -> mode 0 (vertical)
    s.bits("0 011")        # block 3: A = block 2 = 0, B = block 1 = 8 -> predictor 0; rem 3 -> mode 4 (diagonal down-right)
    s.ue(0)                # intra_chroma_pred_mode 0 (DC)
    s.ue(29)               # coded_block_pattern 1 (table 9-4, Intra column: codeNum 29): 8x8 block 0 alone
    s.se(0)                # mb_qp_delta
    # 8x8 block 0: levels 3, -1 at scan positions 0, 1 and 1 at position 5; 4x4 block j takes positions 4k + j (7.3.5.3.2):
    # block 0 = [3], block 1 = [-1, 1], blocks 2 and 3 empty
    s.bits("000101 001 1")   # block 0, nC 0: coeff_token TotalCoeff 1 / T1s 0; level 3: levelCode 4 - 2 = prefix 2; total_zeros 0
    s.bits("001 0 1 111")    # block 1, nC 1 (left 1): TotalCoeff 2 / T1s 2; signs + (position 1), - (position 0); total_zeros 0 of tzVlcIndex 2
    s.bits("1")              # block 2, nC 1 (above 1): TotalCoeff 0
    s.bits("1")              # block 3, nC (0 + 2 + 1) >> 1 = 1: TotalCoeff 0
    # ---- macroblock 1: I_NxN, transform_size_8x8_flag 0; sixteen modes in decoding order.  No row above: B missing in the top row
    s.ue(0).u(1, 0)
    s.bits("0 111")        # 0 (0,0): predictor 2 -> rem 7: mode 8
    s.bits("1")            # 1 (1,0): predictor 2: mode 2
    s.bits("1")            # 2 (0,1): A = left macroblock, 4x4 block 7 -> its 8x8 block 1 = 8; B = block 0 = 8: predictor 8: mode 8
    s.bits("1")            # 3 (1,1): A = 8, B = 2: mode 2
    s.bits("1 1 1 1")      # 4 .. 7: predictor 2 everywhere: mode 2
    s.bits("1")            # 8 (0,2): A = left macroblock, 4x4 block 13 -> its 8x8 block 3 = 4; B = block 2 = 8: predictor 4: mode 4
    s.bits("1")            # 9 (1,2): A = 4, B = block 3 = 2: mode 2
    s.bits("0 001")        # 10 (0,3): A = left 8x8 block 3 = 4, B = block 8 = 4: predictor 4; rem 1 -> mode 1
    s.bits("1")            # 11 (1,3): A = 1, B = 2: mode 1
    s.bits("1 1")          # 12 (2,2), 13 (3,2): mode 2
    s.bits("1 1")          # 14 (2,3): A = block 11 = 1, B = 2: mode 1; 15 (3,3): A = 1, B = 2: mode 1
    s.ue(0)                # intra_chroma_pred_mode 0
    s.ue(3)                # coded_block_pattern 0 (Intra column: codeNum 3)
    p = Parser(quiet=True, lib=lib, intra8x8=True)
    assert p.feed(7, 3, sps) is None and p.feed(8, 3, pps) is None
    pic = p.feed(5, 3, s.rbsp())
    if pic is None:
        pic = p.feed(11, 0, b"")                            # (end of stream closes the picture)
    assert pic is not None and (pic.mb_w, pic.mb_h) == (2, 1)
    rec = pic.mb_records()
    assert pic.desc.transform_8x8 == 3 and pic.desc.slice_type == N.SLICE_I and pic.desc.deblock == 0
    assert rec["mb_type"].tolist() == [N.MB_I4x4, N.MB_I4x4] and rec["intra_modes"].tolist() == [N.MB_I8X8, 0]
    assert rec["qp"].tolist() == [26, 26] and rec["cbp"].tolist() == [1, 0] and rec["coef_mask"].tolist() == [0xF, 0]
    assert rec["avail"].tolist() == [0, N.AVAIL_LEFT] and rec["coef_index"][0] == 0 and pic.desc.n_coef_blocks == 4
    assert pic.i4modes[:16].tolist() == [2] * 4 + [8] * 4 + [0] * 4 + [4] * 4
    assert pic.i4modes[16:].tolist() == [8, 2, 8, 2, 2, 2, 2, 2, 4, 2, 1, 1, 2, 2, 1, 1]
    assert pic.coefs[:64].tolist() == [3, -1, 0, 0, 0, 1] + [0] * 58
    assert lib.p264hip_records_check_pic(pic.desc, pic.desc.mb) == -1
    # the same bits without the option: refused at the flag
    q = Parser(quiet=True, lib=lib)
    q.feed(7, 3, sps), q.feed(8, 3, pps)
    with pytest.raises(Exception):
        if q.feed(5, 3, s.rbsp()) is None:
            raise Exception("no picture")


@pytest.mark.parametrize("case", ["p_cavlc", "p_cabac", "b_cabac_two_slices", "constrained_intra"])
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
        p = Parser(quiet=True, lib=lib, intra8x8=True)
        for typ, idc, rbsp in N.split_annexb(lib, bytes(bad)):
            try:
                pic = p.feed(typ, idc, rbsp)
            except Exception:
                continue
            if pic is not None:
                assert lib.p264hip_records_check_pic(pic.desc, pic.desc.mb) == -1
