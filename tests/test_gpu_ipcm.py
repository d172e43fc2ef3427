"""Streams with I_PCM macroblocks (stream writer: --ipcm) on the MI355X: parsed, reconstructed by the HIP kernels and compared
with tests/pcm_checker.py - bytes of whole planes, every picture of every stream - through p264hip_submit, the drop-in API
(p264_decoder_decode), the command-line decoder and the multi-stream pipeline.  The reference cannot decode these streams
(decoder/macroblock.c:510-514); neither could the parent of this change, whose parser stopped at the first I_PCM macroblock."""
import os
import subprocess

import numpy as np
import pytest

from p264decoder_amd import Decoder, HipReconstructor, Parser, Pipeline, _native as N
from tests import pcm_checker, synth_cases
from tests.test_gpu_cli import CLI
from tests.test_ipcm_cpu import STREAMS, make

pytestmark = pytest.mark.gpu

CIF = "--mbw 22 --mbh 18"
BIG = {
    "1080p_qpd_dbo": "--mbw 120 --mbh 68 --frames 4 --gop 0 --seed 320 --qp 27 --qp-delta 6 --deblock-offsets 3 -2 --coded 12 --maxlevel 8 --ipcm 3",
    "1080p_main_cabac_ipb": "--mbw 120 --mbh 68 --frames 7 --seed 321 --refs 2 --bframes 2 --implicit --d8inf --coded 12 --maxlevel 12 --cabac --ipcm 3",
}


def cif(args):
    a = args.split()
    for k in ("--mbw", "--mbh"):
        i = a.index(k); del a[i:i + 2]
    return CIF + " " + " ".join(a)


def checker_frames(lib, oracle, data):
    """[(Y, U, V)] of every picture of a stream, decode order, by the checker; and the parsed pictures"""
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    chk = pcm_checker.PcmChecker(oracle, pics[0].mb_w, pics[0].mb_h, parser.slots)
    return pics, parser.slots, [[a.copy() for a in chk.reconstruct(p)] for p in pics]


def decode_and_compare(lib, oracle, data, what):
    pics, slots, want = checker_frames(lib, oracle, data)
    hip = HipReconstructor(pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1, lib=lib)
    n_pcm = 0
    for i, (p, w) in enumerate(zip(pics, want)):
        hip.submit(0, p)
        for plane, (a, b) in enumerate(zip(hip.read_frame(0, p.desc.dst_slot), w)):
            assert np.array_equal(a, b), "%s picture %d plane %d: %d samples differ" % (what, i, plane, int((a != b).sum()))
        n_pcm += len(p.ipcm_macroblocks())
    hip.close()
    assert n_pcm > 20
    return pics


@pytest.mark.parametrize("cabac", [False, True], ids=["cavlc", "cabac"])
@pytest.mark.parametrize("name", list(STREAMS))
def test_ipcm_streams_cif(lib, oracle, tmp_path, name, cabac):
    decode_and_compare(lib, oracle, make(tmp_path, cif(STREAMS[name]) + (" --cabac" if cabac else ""), "s"), name)


@pytest.mark.parametrize("name", list(BIG))
def test_ipcm_streams_1080p(lib, oracle, tmp_path, name):
    pics = decode_and_compare(lib, oracle, make(tmp_path, BIG[name], "s"), name)
    if "qpd" in name:
        assert len({int(q) for p in pics for q in p.mb_records()["qp"]}) > 8       # QP 0 of the I_PCM records among the chain's QPs


def test_ipcm_through_the_dropin_api(lib, oracle, tmp_path):
    data = make(tmp_path, cif(STREAMS["b_spatial"]) + " --cabac", "s")
    _, _, want = checker_frames(lib, oracle, data)
    dec = Decoder(lib=lib)
    got = list(dec.decode_annexb(data))
    dec.close()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):               # (pictures come out in decode order, like the reference's)
        for plane in range(3):
            assert np.array_equal(g[plane], w[plane]), "picture %d plane %d" % (i, plane)


def test_ipcm_through_the_cli(lib, oracle, tmp_path):
    data = make(tmp_path, cif(STREAMS["qp_delta"]), "in")
    _, _, want = checker_frames(lib, oracle, data)
    out = tmp_path / "out.yuv"
    r = subprocess.run([CLI, "-d", str(tmp_path / "in.264"), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b"".join(pl.tobytes() for f in want for pl in f)


def test_ipcm_through_the_pipeline(lib, oracle, tmp_path):
    with_pcm = make(tmp_path, cif(STREAMS["ip_baseline"]), "a")
    with_pcm_cabac = make(tmp_path, cif(STREAMS["slices3"]) + " --cabac", "b")
    plain = synth_cases.stream_bytes("cif_ip")
    streams = [with_pcm, plain, with_pcm_cabac, with_pcm, plain]
    last = {id(s): checker_frames(lib, oracle, s)[2][-1] for s in (with_pcm, plain, with_pcm_cabac)}
    pipe = Pipeline(streams, threads=4, device=0, lib=lib)
    st = pipe.run()
    assert st["pictures"] == 8 + 24 + 8 + 8 + 24
    for i, s in enumerate(streams):
        for plane, (a, b) in enumerate(zip(pipe.read_frame(i), last[id(s)])):
            assert np.array_equal(a, b), "stream %d plane %d" % (i, plane)
    pipe.close()
