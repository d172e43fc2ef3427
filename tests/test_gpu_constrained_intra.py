"""Streams with constrained_intra_pred_flag (stream writer: --constrained-intra) on the MI355X: parsed, reconstructed by the HIP
kernels and compared with tests/intra_checker.py - bytes of whole planes, every picture of every stream - through
p264hip_submit, the drop-in API (p264_decoder_decode) and the command-line decoder.  The reference ignores the flag
(decoder/set.c:241) and so did the parent of this change.  What these tests pin is what the kernels do with the availability
the flag produces (LEFT, TOP and no TOPLEFT among it: twelve of the thirteen fail on the parent's kernels); a misread flag they
cannot see - kernels and checker get the same records - unless it makes a mode illegal, which the checker refuses: the parser's
reading is pinned by tests/test_constrained_intra_cpu.py against the stream writer's record."""
from functools import partial

import pytest

from p264decoder_amd import _native as N
from tests import hip_harness as H
from tests import intra_checker
from tests.stream_args import CI, CI_STREAMS as STREAMS, cif
from tests.synth_cases import write_stream as write

pytestmark = pytest.mark.gpu

BIG = "--mbw 120 --mbh 68 --frames 3 --gop 0 --seed 420 --qp 27 --qp-delta 5 --coded 12 --maxlevel 8 --ipcm 2 --constrained-intra --intra-pct 15"


def submit_and_count_flags(lib, oracle, data, what):
    pics, slots, want, _ = H.parse_and_expect(lib, data, partial(intra_checker.IntraChecker, oracle))
    H.submit_stream(lib, pics, slots, want, what)
    flags = set()
    for p in pics:
        if p.desc.slice_type != N.SLICE_I:
            r = p.mb_records()
            flags |= {int(a) for a in r["avail"][r["mb_type"] <= N.MB_IPCM]}
    assert len(flags) >= 14, "only %d of the sixteen flag combinations on intra macroblocks of P / B pictures" % len(flags)


@pytest.mark.parametrize("cabac", [False, True], ids=["cavlc", "cabac"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_constrained_intra_streams_cif(lib, oracle, tmp_path, name, cabac):
    submit_and_count_flags(lib, oracle, write(tmp_path, cif(STREAMS[name]) + CI + (" --cabac" if cabac else "")), name)


def test_constrained_intra_stream_1080p(lib, oracle, tmp_path):
    submit_and_count_flags(lib, oracle, write(tmp_path, BIG), "1080p")


def test_constrained_intra_through_the_dropin_api(lib, oracle, tmp_path):
    data = write(tmp_path, cif(STREAMS["b"]) + CI + " --cabac")
    _, _, want, _ = H.parse_and_expect(lib, data, partial(intra_checker.IntraChecker, oracle))
    H.compare_pictures(H.dropin_pictures(lib, data), want, "drop-in decoder")      # (decode order, like the reference's)


def test_constrained_intra_through_the_cli(lib, oracle, tmp_path):
    data = write(tmp_path, cif(STREAMS["slices3"]) + CI, "in")
    _, _, want, _ = H.parse_and_expect(lib, data, partial(intra_checker.IntraChecker, oracle))
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want)
