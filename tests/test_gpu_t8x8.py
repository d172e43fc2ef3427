"""The 8x8 transform of inter macroblocks on the MI355X: the pictures of tests/t8x8_stim.py through p264hip_submit, through
p264hip_upload + p264hip_reconstruct in batches of three and through the compact road, all three planes byte for byte against
tests/t8x8_checker.py (H.264 8.5.6, 8.5.9, 8.5.13, 8.7 - the oracle does not know the flag); batches that mix flagged and
unflagged pictures; what the launch reports; the refusals of the seam on the device roads."""

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor, _native as N
from p264decoder_amd.recon import P264Error
from tests import inter_stim
from tests import spec_recon
from tests import t8x8_checker as T8
from tests import t8x8_stim as TS
from tests.test_gpu_inter_spec import by_size, differences

pytestmark = pytest.mark.gpu
SLOTS = 3


def expect(st, cls=T8.SpecRecon):
    spec = cls(st.pic.mb_w, st.pic.mb_h, SLOTS)
    for slot, f in st.frames.items():
        spec.store.write(slot, f)
    return [p.copy() for p in spec.reconstruct(st.pic)]


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    return {which: [(st, expect(st)) for st in getattr(TS, which)()] for which in TS.SETS}


@pytest.mark.parametrize("which", TS.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    bad, sent = [], []
    for (mb_w, mb_h), cases in by_size(expected[which]).items():
        hip = HipReconstructor(mb_w, mb_h, n_streams=1, slots=SLOTS, max_pictures=1, lib=lib)
        for st, want in cases:
            for slot, f in st.frames.items():
                hip.write_frame(0, slot, *f)
            hip.submit(0, st.pic)
            assert hip.last_t8x8_wgs() == (mb_w * mb_h + 7) // 8
            bad += differences(hip.read_frame(0, st.pic.desc.dst_slot), want, st.name, st.pic)
            sent.append(st)
        hip.close()
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    TS.assert_covered(which, sent)


def run_batches(lib, cases, n=3, road="upload"):
    """the cases (one picture size) in batches of n distinct pictures, one stream each"""
    (mb_w, mb_h), = {(st.pic.mb_w, st.pic.mb_h) for st, _ in cases}
    hip = HipReconstructor(mb_w, mb_h, n_streams=n, slots=SLOTS, max_pictures=n, lib=lib)
    bad, sent, wgs = [], [], []
    for at in range(0, len(cases), n):
        batch = [cases[(at + k) % len(cases)] for k in range(n)]
        assert len({id(st.pic) for st, _ in batch}) == n
        for k, (st, _) in enumerate(batch):
            for slot, f in st.frames.items():
                hip.write_frame(k, slot, *f)
        if road == "upload":
            hip.upload(0, [st.pic for st, _ in batch])
        else:
            for k, (st, _) in enumerate(batch):
                hip.upload_compact(k, st.pic, HipReconstructor.pack_compact(st.pic, lib))
        hip.reconstruct(list(range(n)), list(range(n)))
        wgs.append((hip.last_t8x8_wgs(), any(st.pic.desc.transform_8x8 for st, _ in batch)))
        for k, (st, want) in enumerate(batch):
            bad += differences(hip.read_frame(k, st.pic.desc.dst_slot), want, "%s (stream %d of a batch, %s)" % (st.name, k, road), st.pic)
            sent.append(st)
    hip.close()
    return bad, sent, wgs


@pytest.mark.parametrize("road", ["upload", "compact"])
def test_batches_of_three_equal_the_standard(lib, expected, road):
    cases = by_size(expected["directed_set"] + expected["random_set"])[(TS.MB_W, TS.MB_H)]
    bad, sent, wgs = run_batches(lib, cases, road=road)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(w == 3 * ((TS.MB_W * TS.MB_H + 7) // 8) for w, _ in wgs)
    directed = {id(st.pic) for st, _ in expected["directed_set"]}
    TS.assert_covered("directed_set", [st for st in {id(st.pic): st for st in sent}.values() if id(st.pic) in directed])


def test_mixed_batches_and_what_the_launch_reports(lib, expected):
    """flagged P, flagged B, explicit-weight and unflagged pictures in one batch; a batch without a flagged picture does not
    launch k_t8x8 (and decodes as ever), one with a flagged picture does"""
    d = {st.name: (st, want) for st, want in expected["directed_set"]}
    plain = [(st, expect(st, spec_recon.SpecRecon)) for st in inter_stim.window_set()[:2] + inter_stim.b_set()[:1] + inter_stim.weighted_set()[:1]]
    assert not any(st.pic.desc.transform_8x8 for st, _ in plain)
    mixed = [d["P shapes"], plain[2], d["mixed P weighted 0"], plain[0], d["B implicit road by road"], plain[3], d["mixed B weighted 1"], plain[1], d["quadrants"]]
    bad, sent, wgs = run_batches(lib, mixed)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert all(w > 0 for w, _ in wgs)
    kinds = {(int(st.pic.desc.slice_type), bool(st.pic.desc.explicit_wp), bool(st.pic.desc.transform_8x8)) for st in sent}
    assert kinds >= {(N.SLICE_P, False, True), (N.SLICE_B, False, True), (N.SLICE_P, True, True), (N.SLICE_P, False, False), (N.SLICE_B, False, False)}
    bad, sent, wgs = run_batches(lib, plain[:3])
    assert not bad and wgs == [(0, False)]


def test_the_device_roads_refuse_what_the_seam_forbids(lib, expected):
    st, want = next(c for c in expected["directed_set"] if c[0].name.startswith("mixed P"))
    pic, rec = st.pic, st.pic.mb_records()
    fl = np.flatnonzero((rec["intra_modes"] & N.MB_T8X8) != 0)
    coded = next(int(m) for m in fl if rec["coef_mask"][m] & 0xffff)
    intra = int(np.flatnonzero(rec["mb_type"] <= N.MB_I16x16)[0])
    hip = HipReconstructor(pic.mb_w, pic.mb_h, n_streams=1, slots=SLOTS, max_pictures=2, lib=lib)
    for slot, f in st.frames.items():
        hip.write_frame(0, slot, *f)
    good = HipReconstructor.pack(pic, lib)
    mask = int(rec["coef_mask"][coded])
    k = next(k for k in range(4) if mask >> (4 * k) & 1)
    for m, field, value, t8 in ((coded, "coef_mask", mask & ~(2 << (4 * k)), 1), (intra, "intra_modes", int(rec["intra_modes"][intra]) | N.MB_T8X8, 1),
                                (int(fl[0]), "qp", int(rec["qp"][fl[0]]), 0)):
        keep = rec[field][m]
        rec[field][m], pic.desc.transform_8x8 = value, t8
        try:
            with pytest.raises(P264Error):                      # p264hip_upload checks on the host
                hip.upload(1, [pic])
            bad = good.copy()
            bad[16 * m:16 * m + 16] = np.frombuffer(rec[m:m + 1].tobytes(), np.uint8)
            dev, n = hip.input_reserve(0, pic)                  # reserve / commit: the check runs on the device
            assert n == bad.size and lib.p264hip_copy_to_device(dev, bad.ctypes.data, n) == 0
            hip.input_commit(0)
            with pytest.raises(P264Error):
                hip.reconstruct([0], [0])
        finally:
            rec[field][m], pic.desc.transform_8x8 = keep, 1
    dev, n = hip.input_reserve(0, pic)
    assert lib.p264hip_copy_to_device(dev, good.ctypes.data, n) == 0
    hip.input_commit(0)
    hip.reconstruct([0], [0])
    assert not differences(hip.read_frame(0, pic.desc.dst_slot), want, "the good picture behind the refused ones", pic)
    hip.close()


# ---- a whole stream ------------------------------------------------------------------------------------------------------------
STREAM = "--mbw 8 --mbh 6 --frames 10 --refs 2 --bframes 2 --d8inf --cabac --t8x8 70 --qp 14 --qp-delta 3 --coded 35 --maxlevel 3 --seed 85"


def stream_and_standard(lib):
    """(Annex-B bytes, the parser's pictures, the parser's slots, per picture [y, u, v] by the checker run picture after picture
    on its own frame store)"""
    from p264decoder_amd import Parser
    from tests import synth_cases
    data = open(synth_cases.generate(STREAM), "rb").read()
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    spec = T8.SpecRecon(pics[0].mb_w, pics[0].mb_h, parser.slots)
    want = [[a.copy() for a in spec.reconstruct(p)] for p in pics]
    return data, pics, parser.slots, want, spec


def test_a_high_profile_cabac_b_stream_end_to_end(lib, tmp_path):
    """synth264 --t8x8 (High profile, CABAC, P and B pictures) through the parser and p264hip_submit, through the drop-in decoder
    and through the command-line decoder: every picture equals the standard's"""
    import os
    import subprocess
    from p264decoder_amd import Decoder, build as _build
    data, pics, slots, want, spec = stream_and_standard(lib)
    assert len(pics) == 10 and {int(p.desc.slice_type) for p in pics} == {N.SLICE_I, N.SLICE_P, N.SLICE_B}
    flagged = [int(((p.mb_records()["intra_modes"] & N.MB_T8X8) != 0).sum()) for p in pics]
    assert all(p.desc.transform_8x8 for p in pics) and sum(flagged) >= 60 and sum(f > 0 for f in flagged) >= 7, flagged
    assert spec.tells["v"] + spec.tells["h"] > 0
    hip = HipReconstructor(pics[0].mb_w, pics[0].mb_h, n_streams=1, slots=slots, max_pictures=1, lib=lib)
    for i, (p, w) in enumerate(zip(pics, want)):
        hip.submit(0, p)
        assert not differences(hip.read_frame(0, p.desc.dst_slot), w, "picture %d" % i, p)
    hip.close()
    dec = Decoder(lib=lib)
    got = [[np.array(a) for a in pic] for pic in dec.decode_annexb(data)]
    dec.close()
    assert len(got) == 10
    for i, (g, w) in enumerate(zip(got, want)):
        for plane, (a, b) in enumerate(zip(g, w)):
            assert np.array_equal(a[:b.shape[0], :b.shape[1]], b), "drop-in decoder: picture %d plane %d" % (i, plane)
    cli = os.path.join(os.path.dirname(_build.__file__), "tools", "p264decoder_amd")
    src, out = tmp_path / "t8.264", tmp_path / "rec.yuv"
    src.write_bytes(data)
    r = subprocess.run([cli, "-d", str(src), str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    frame = b"".join(b"".join(pl.tobytes() for pl in w) for w in want)
    assert raw == frame, "the command-line decoder's pictures differ from the standard's"
