"""Streams with I_PCM macroblocks (stream writer: --ipcm) on the MI355X: parsed, reconstructed by the HIP kernels and compared
with tests/pcm_checker.py - bytes of whole planes, every picture of every stream - through p264hip_submit, the drop-in API
(p264_decoder_decode), the command-line decoder and the multi-stream pipeline.  The reference cannot decode these streams
(decoder/macroblock.c:510-514); neither could the parent of this change, whose parser stopped at the first I_PCM macroblock."""
from functools import partial

import pytest

from p264decoder_amd import Pipeline
from tests import hip_harness as H
from tests import pcm_checker, synth_cases
from tests.stream_args import IPCM_STREAMS as STREAMS, cif
from tests.synth_cases import write_stream as make

pytestmark = pytest.mark.gpu

BIG = {
    "1080p_qpd_dbo": "--mbw 120 --mbh 68 --frames 4 --gop 0 --seed 320 --qp 27 --qp-delta 6 --deblock-offsets 3 -2 --coded 12 --maxlevel 8 --ipcm 3",
    "1080p_main_cabac_ipb": "--mbw 120 --mbh 68 --frames 7 --seed 321 --refs 2 --bframes 2 --implicit --d8inf --coded 12 --maxlevel 12 --cabac --ipcm 3",
}


def submit_and_count_ipcm(lib, oracle, data, what):
    pics, slots, want, _ = H.parse_and_expect(lib, data, partial(pcm_checker.PcmChecker, oracle))
    H.submit_stream(lib, pics, slots, want, what)
    assert sum(len(p.ipcm_macroblocks()) for p in pics) > 20
    return pics


@pytest.mark.parametrize("cabac", [False, True], ids=["cavlc", "cabac"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_ipcm_streams_cif(lib, oracle, tmp_path, name, cabac):
    submit_and_count_ipcm(lib, oracle, make(tmp_path, cif(STREAMS[name]) + (" --cabac" if cabac else ""), "s"), name)


@pytest.mark.parametrize("name", list(BIG))
def test_ipcm_streams_1080p(lib, oracle, tmp_path, name):
    pics = submit_and_count_ipcm(lib, oracle, make(tmp_path, BIG[name], "s"), name)
    if "qpd" in name:
        assert len({int(q) for p in pics for q in p.mb_records()["qp"]}) > 8       # QP 0 of the I_PCM records among the chain's QPs


def test_ipcm_through_the_dropin_api(lib, oracle, tmp_path):
    data = make(tmp_path, cif(STREAMS["b_spatial"]) + " --cabac", "s")
    _, _, want, _ = H.parse_and_expect(lib, data, partial(pcm_checker.PcmChecker, oracle))
    H.compare_pictures(H.dropin_pictures(lib, data), want, "drop-in decoder")      # (decode order, like the reference's)


def test_ipcm_through_the_cli(lib, oracle, tmp_path):
    data = make(tmp_path, cif(STREAMS["qp_delta"]), "in")
    _, _, want, _ = H.parse_and_expect(lib, data, partial(pcm_checker.PcmChecker, oracle))
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want)


def test_ipcm_through_the_pipeline(lib, oracle, tmp_path):
    with_pcm = make(tmp_path, cif(STREAMS["ip_baseline"]), "a")
    with_pcm_cabac = make(tmp_path, cif(STREAMS["slices3"]) + " --cabac", "b")
    plain = synth_cases.stream_bytes("cif_ip")
    streams = [with_pcm, plain, with_pcm_cabac, with_pcm, plain]
    last = {id(s): H.parse_and_expect(lib, s, partial(pcm_checker.PcmChecker, oracle))[2][-1] for s in (with_pcm, plain, with_pcm_cabac)}
    pipe = Pipeline(streams, threads=4, device=0, lib=lib)
    st = pipe.run()
    assert st["pictures"] == 8 + 24 + 8 + 8 + 24
    for i, s in enumerate(streams):
        H.compare(pipe.read_frame(i), last[id(s)], "stream %d" % i)
    pipe.close()
