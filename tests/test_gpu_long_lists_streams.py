"""Streams whose reference lists grow to 16 entries in a store of 17 slots (tests/stream_args.py: LONG_LISTS;
tests/test_long_lists_streams_cpu.py ties their parse to the stream writer's records), on the GPU: every picture of every stream
through upload and reconstruct, through the drop-in decoder and - three streams side by side - through the pipeline, one stream
through the command-line decoder; byte for byte the pictures tests/spec_recon.py gives for the parsed pictures, decoded picture
after picture on its own frame store."""
import pytest

from p264decoder_amd import Pipeline, _native as N
from tests import hip_harness as H
from tests import spec_recon, synth_cases
from tests.stream_args import LONG_LISTS

pytestmark = pytest.mark.gpu

NAMES = list(LONG_LISTS)
PIPELINE = ("p_cavlc_mmco", "b_cabac_temporal", "b_cavlc_wp_8")


@pytest.fixture(scope="module")
def streams(lib):
    """{name: (stream bytes, pictures, slots, [y, u, v] per picture by the standard)}, computed once"""
    out = {}
    for name, args in LONG_LISTS.items():
        data = open(synth_cases.generate(args), "rb").read()
        pics, slots, want, _ = H.parse_and_expect(lib, data, spec_recon.SpecRecon)
        out[name] = (data, pics, slots, want)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_upload_and_reconstruct_equal_the_standard(lib, streams, name):
    data, pics, slots, want = streams[name]
    refs = int(LONG_LISTS[name].split("--refs ")[1].split()[0])
    assert slots == refs + 1 and max(int(p.desc.n_ref) for p in pics) == refs
    full = 0
    with H.reconstructor(lib, pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1) as hip:
        for i, (p, w) in enumerate(zip(pics, want)):
            hip.upload(0, [p])
            hip.reconstruct([0], [0])
            H.compare(hip.read_frame(0, p.desc.dst_slot), w, "%s picture %d" % (name, i), p)
            full += int(p.desc.n_ref) == refs and (p.desc.slice_type != N.SLICE_B or int(p.desc.n_ref_l1) == refs)
    assert full >= 4, "%s: only %d pictures with full lists" % (name, full)


@pytest.mark.parametrize("name", NAMES)
def test_the_drop_in_decoder_gives_the_same_pictures(lib, streams, name):
    data, pics, _, want = streams[name]
    got = H.dropin_pictures(lib, data)
    assert len(got) == len(pics)
    H.compare_pictures(got, want, "%s: drop-in decoder" % name, crop=True)


def test_three_streams_side_by_side_in_the_pipeline(lib, streams):
    """different lengths, 17 and 9 slots, P / B, CAVLC / CABAC in one pipeline: the picture every stream ends with, then - a second
    pipeline, stopped after 57 pictures - a B picture of the longest stream with 16 + 16 entries"""
    for limit in (0, 57):
        pipe = Pipeline([streams[n][0] for n in PIPELINE], threads=3, device=0, lib=lib)
        try:
            st = pipe.run(max_pictures=limit) if limit else pipe.run()
            lengths = [min(len(streams[n][1]), limit or 10 ** 9) for n in PIPELINE]
            assert st["pictures"] == sum(lengths), st
            for i, n in enumerate(PIPELINE):
                last = lengths[i] - 1
                H.compare(pipe.read_frame(i), streams[n][3][last], "%s: picture %d of the pipeline's stream %d" % (n, last, i), streams[n][1][last])
        finally:
            pipe.close()
    mid = streams["b_cabac_temporal"][1][56].desc
    assert mid.slice_type == N.SLICE_B and (int(mid.n_ref), int(mid.n_ref_l1)) == (16, 16)


def test_the_command_line_decoder_gives_the_same_pictures(lib, streams, tmp_path):
    data, _, _, want = streams["p_cavlc"]
    assert H.cli_bytes(tmp_path, data) == H.planes_bytes(want), "the command-line decoder's pictures differ from the standard's"
