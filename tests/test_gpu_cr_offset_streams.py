"""Whole streams whose PPS gives Cr a QP offset of its own (synth264 --cqo 3 --cqo2 -7; CAVLC P pictures, CABAC with B pictures; 7
pictures of 11 x 9 macroblocks, High profile with the 8x8 transform) against the two-chain composite of tests/cr_offset_checker.py in
decode order: through the parser and p264hip_submit, through the pipeline (the last frame read back, and exported as I420) and through
the drop-in decoder."""
import numpy as np
import pytest

from p264decoder_amd import Pipeline
from p264decoder_amd import _native as N
from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import export_checker as X
from tests import hip_harness as H
from tests import scaling_checker as SC
from tests import synth_cases
from tests.device_mem import DeviceBuffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=list(CS.STREAMS))
def stream(request, lib):
    data = open(synth_cases.generate(CS.stream_args(request.param)), "rb").read()
    pics, slots, want, two = H.parse_and_expect(lib, data, lambda w, h, s: CR.TwoChains(SC.SpecRecon, w, h, s), intra8x8=True, scaling=True, cr_offset=True)
    assert len(pics) == 7 and all((int(p.desc.chroma_qp_offset), CR.delta_of(p)) == (CS.CQO, CS.CQO2 - CS.CQO) for p in pics)
    assert two.v_differs == 7
    types = {int(p.desc.slice_type) for p in pics}
    assert types == ({N.SLICE_I, N.SLICE_P, N.SLICE_B} if "--bframes" in CS.STREAMS[request.param] else {N.SLICE_I, N.SLICE_P})
    for i, p in enumerate(pics):
        for cr in (False, True):
            with CR.variant(p, cr):
                n, out = SC.census(p)
            assert n and not out, "picture %d: level blocks out of range: %s" % (i, sorted(out)[:3])
    return data, pics, slots, want


def test_submit(lib, stream):
    data, pics, slots, want = stream

    def probe(hip, i, p):
        assert (hip.last_cr_pictures(), hip.last_scaled_pictures()) == (1, 1)
    H.submit_stream(lib, pics, slots, want, "p264hip_submit", probe)


def test_the_drop_in_decoder(lib, stream):
    data, pics, slots, want = stream
    got = H.dropin_pictures(lib, data)
    assert len(got) == 7
    H.compare_pictures(got, want, "drop-in decoder", crop=True)


def test_the_pipeline(lib, stream):
    data, pics, slots, want = stream
    pipe = Pipeline([data, data], threads=2, device=0, lib=lib)
    try:
        st = pipe.run()
        assert st["pictures"] == 14 and [pipe.pictures(s) for s in range(2)] == [7, 7]
        for s in range(2):
            H.compare(pipe.read_frame(s), want[-1], "pipeline stream %d" % s, pics[-1])
        w, h = pics[0].mb_w * 16, pics[0].mb_h * 16
        per = X.frame_bytes("i420", w, h)
        last = DeviceBuffer(lib, 2 * per)
        try:
            pipe.export_last("i420", out=(last.ptr, 2 * per))
            assert np.array_equal(last.host(), X.expected([want[-1], want[-1]], "i420", (0, 0, w, h)))
        finally:
            last.free()
    finally:
        pipe.close()
