"""Streams with constrained_intra_pred_flag (stream writer: --constrained-intra) on the MI355X: parsed, reconstructed by the HIP
kernels and compared with tests/intra_checker.py - bytes of whole planes, every picture of every stream - through
p264hip_submit, the drop-in API (p264_decoder_decode) and the command-line decoder.  The reference ignores the flag
(decoder/set.c:241) and so did the parent of this change.  What these tests pin is what the kernels do with the availability
the flag produces (LEFT, TOP and no TOPLEFT among it: twelve of the thirteen fail on the parent's kernels); a misread flag they
cannot see - kernels and checker get the same records - unless it makes a mode illegal, which the checker refuses: the parser's
reading is pinned by tests/test_constrained_intra_cpu.py against the stream writer's record."""
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Decoder, HipReconstructor, Parser, _native as N
from tests import intra_checker
from tests.test_constrained_intra_cpu import CI, STREAMS, write
from tests.test_gpu_cli import CLI
from tests.test_gpu_ipcm import cif

pytestmark = pytest.mark.gpu

BIG = "--mbw 120 --mbh 68 --frames 3 --gop 0 --seed 420 --qp 27 --qp-delta 5 --coded 12 --maxlevel 8 --ipcm 2 --constrained-intra --intra-pct 15"


def checker_frames(lib, oracle, data):
    """[(Y, U, V)] of every picture of a stream, decode order, by the intra checker; and the parsed pictures"""
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    chk = intra_checker.IntraChecker(oracle, pics[0].mb_w, pics[0].mb_h, parser.slots)
    return pics, parser.slots, [[a.copy() for a in chk.reconstruct(p)] for p in pics]


def decode_and_compare(lib, oracle, data, what):
    pics, slots, want = checker_frames(lib, oracle, data)
    hip = HipReconstructor(pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1, lib=lib)
    flags = set()
    for i, (p, w) in enumerate(zip(pics, want)):
        hip.submit(0, p)
        for plane, (a, b) in enumerate(zip(hip.read_frame(0, p.desc.dst_slot), w)):
            assert np.array_equal(a, b), "%s picture %d plane %d: %d samples differ" % (what, i, plane, int((a != b).sum()))
        if p.desc.slice_type != N.SLICE_I:
            r = p.mb_records()
            flags |= {int(a) for a in r["avail"][r["mb_type"] <= N.MB_IPCM]}
    hip.close()
    assert len(flags) >= 14, "only %d of the sixteen flag combinations on intra macroblocks of P / B pictures" % len(flags)


@pytest.mark.parametrize("cabac", [False, True], ids=["cavlc", "cabac"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_constrained_intra_streams_cif(lib, oracle, tmp_path, name, cabac):
    decode_and_compare(lib, oracle, write(tmp_path, cif(STREAMS[name]) + CI + (" --cabac" if cabac else "")), name)


def test_constrained_intra_stream_1080p(lib, oracle, tmp_path):
    decode_and_compare(lib, oracle, write(tmp_path, BIG), "1080p")


def test_constrained_intra_through_the_dropin_api(lib, oracle, tmp_path):
    data = write(tmp_path, cif(STREAMS["b"]) + CI + " --cabac")
    _, _, want = checker_frames(lib, oracle, data)
    dec = Decoder(lib=lib)
    got = list(dec.decode_annexb(data))
    dec.close()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):               # (pictures come out in decode order, like the reference's)
        for plane in range(3):
            assert np.array_equal(g[plane], w[plane]), "picture %d plane %d" % (i, plane)


def test_constrained_intra_through_the_cli(lib, oracle, tmp_path):
    data = write(tmp_path, cif(STREAMS["slices3"]) + CI, "in")
    _, _, want = checker_frames(lib, oracle, data)
    out = tmp_path / "out.yuv"
    r = subprocess.run([CLI, "-d", str(tmp_path / "in.264"), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b"".join(pl.tobytes() for f in want for pl in f)
