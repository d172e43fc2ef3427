"""Streams whose slices differ in reference lists and loop-filter offsets (tests/slice_streams.py) on the MI355X, through every
road that takes what the parser publishes: HipReconstructor picture by picture, the drop-in Decoder, the command-line decoder and
the Pipeline.  Expected pictures: the oracle's unfiltered reconstruction followed by tests/slice_filter_checker.py - the oracle's
own filter knows one offset pair per picture - compared byte for byte."""
import os

import numpy as np
import pytest

from p264decoder_amd import Pipeline
from tests import hip_harness as H
from tests import slice_streams as ss

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name", list(ss.STREAMS))
def test_streams_through_the_reconstructor(lib, oracle, tmp_path, name):
    data, dump = ss.make(tmp_path, ss.STREAMS[name])
    parser, pics = ss.parse(lib, data)
    ss.check_against_dump(pics, dump)
    want = ss.expected_pictures(oracle, pics, parser.slots)
    with H.reconstructor(lib, pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=parser.slots, max_pictures=1) as hip:
        for i, p in enumerate(pics):
            if i % 2:
                hip.submit(0, p)
            else:
                H.put(hip, lib, 0, p, "compact")
                hip.reconstruct([0], [0])
            H.compare(hip.read_frame(0, p.desc.dst_slot), want[i], "%s picture %d (slice type %d)" % (name, i, p.desc.slice_type), p)


@pytest.mark.parametrize("name", ["p_cabac_3", "b_cavlc_temporal_4"])
def test_streams_through_the_dropin_decoder(lib, oracle, tmp_path, name):
    data, _ = ss.make(tmp_path, ss.STREAMS[name])
    parser, pics = ss.parse(lib, data)
    want = ss.expected_pictures(oracle, pics, parser.slots)
    H.compare_pictures(H.dropin_pictures(lib, data), want, name)      # (pictures come out in decode order)


def test_a_stream_through_the_cli(lib, oracle, tmp_path):
    data, _ = ss.make(tmp_path, ss.STREAMS["p_cavlc_4_sub8x8"])
    parser, pics = ss.parse(lib, data)
    want = ss.expected_pictures(oracle, pics, parser.slots)
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want)


def test_streams_through_the_pipeline(lib, oracle, tmp_path):
    """streams of one geometry and one frame-store size side by side: CAVLC, CABAC, and one whose slices agree"""
    geo = "--mbw 9 --mbh 7 --refs 3 "
    args = [geo + "--frames 11 --seed 131 --bframes 1 --slices 3 --coded 15 --maxlevel 6 --qp 34 " + ss.BOTH,
            geo + "--frames 13 --seed 132 --bframes 2 --implicit --slices 2 --cabac --coded 10 --maxlevel 6 --qp 34 " + ss.BOTH,
            geo + "--frames 9 --seed 133 --bframes 1 --slices 2 --coded 15 --maxlevel 6"]
    streams, last, n_pics = [], [], 0
    for k, a in enumerate(args):
        d = tmp_path / ("s%d" % k)
        d.mkdir()
        data, _ = ss.make(d, a)
        parser, pics = ss.parse(lib, data)
        streams.append(data)
        last.append(ss.expected_pictures(oracle, pics, parser.slots)[-1])
        n_pics += len(pics)
    order = [0, 1, 2, 1, 0]
    pipe = Pipeline([streams[k] for k in order], threads=4, device=0, lib=lib)
    st = pipe.run()
    assert st["pictures"] == 11 + 13 + 9 + 13 + 11
    for i, k in enumerate(order):
        H.compare(pipe.read_frame(i), last[k], "stream %d" % i)
    pipe.close()


def test_streams_through_the_fanout(lib, oracle, tmp_path):
    """two ranks on the box's MI355X, TCP transport: rank 0 parses and scatters the packed pictures (records with their deltas,
    remapped indices), both reconstruct, rank 0 gathers - every picture of every stream"""
    import hashlib
    from tests import fan_helpers
    geo = "--mbw 9 --mbh 7 "
    args = [geo + "--frames 10 --gop 10 --seed 141 --refs 2 --slices 3 --cabac --coded 15 --maxlevel 6 --qp 34 " + ss.BOTH,
            geo + "--frames 10 --seed 142 --refs 3 --bframes 2 --slices 2 --coded 10 --maxlevel 6 --qp 34 " + ss.BOTH]
    streams, want = [], []
    for k, a in enumerate(args):
        d = tmp_path / ("f%d" % k)
        d.mkdir()
        data, _ = ss.make(d, a)
        parser, pics = ss.parse(lib, data)
        streams.append(data)
        want.append([hashlib.sha256(b"".join(np.ascontiguousarray(pl).tobytes() for pl in f)).hexdigest() for f in ss.expected_pictures(oracle, pics, parser.slots)])
    order = [0, 1, 1, 0]
    got, st = fan_helpers.run_job(2, [streams[k] for k in order], 10, False, 29500 + (os.getpid() % 150))
    assert st["pictures"] == 40 and st["pictures_remote"] == 20
    for s, k in enumerate(order):
        for i in range(10):
            assert got[(s, i)] == want[k][i], "stream %d picture %d" % (s, i)
