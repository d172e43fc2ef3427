"""The pure parts of tests/hip_harness.py and synth_cases.write_stream, without a device: the plane comparer on both picture
classes, the batching, the roads into an input slot against a recording stand-in, the stream writer against the cached one."""
import types

import numpy as np
import pytest

from tests import hip_harness as H
from tests import seam_fuzz, synth_cases


class ParsedLike:
    """what first_difference reads of a recon.ParsedPicture: mb_records() and mv, no .rec"""

    def __init__(self, seam):
        self.mv, self._rec = seam.mv, seam.rec

    def mb_records(self):
        return self._rec


@pytest.fixture(params=["seam", "parsed"])
def pic(request):
    seam = seam_fuzz.make_picture(np.random.default_rng(5), 2, 2, p_picture=False)
    seam.rec["qp"][:] = [30, 31, 32, 33]
    return seam if request.param == "seam" else ParsedLike(seam)


def planes():
    return [np.full((32, 32), 7, np.uint8), np.full((16, 16), 8, np.uint8), np.full((16, 16), 9, np.uint8)]


def test_equal_planes_are_no_difference(pic):
    assert H.first_difference(planes(), planes(), "x", pic) is None
    assert H.differences(planes(), planes(), "x", pic) == []
    H.compare(planes(), planes(), "x", pic)


def test_a_luma_sample_names_its_macroblock_and_both_values(pic):
    got = planes()
    got[0][17, 0] = 200
    d = H.first_difference(got, planes(), "case", pic)
    assert d.startswith("case plane 0: 1 samples differ, first (y=17, x=0) macroblock 2 ") and d.endswith(": got 200 want 7")
    assert " qp 32 " in d and "type %d " % pic.mb_records()["mb_type"][2] in d
    assert H.differences(got, planes(), "case", pic) == [d]
    with pytest.raises(pytest.fail.Exception, match="macroblock 2"):
        H.compare(got, planes(), "case", pic)
    assert "macroblock 2:" in H.first_difference(got, planes(), "case")          # without a picture: no record, the same index


def test_a_chroma_sample_counts_macroblocks_on_the_8_sample_grid(pic):
    got = planes()
    got[1][8, 9] = 0
    d = H.first_difference(got, planes(), "case", pic)
    assert "plane 1: 1 samples differ, first (y=8, x=9) macroblock 3 " in d and " qp 33 " in d and d.endswith(": got 0 want 8")


def test_two_differences_report_the_count_and_the_first_in_raster_order(pic):
    got = planes()
    got[0][20, 3] = 1
    got[0][5, 30] = 2
    d = H.first_difference(got, planes(), "case", pic)
    assert "plane 0: 2 samples differ, first (y=5, x=30) macroblock 1 " in d and d.endswith(": got 2 want 7")


def test_a_plane_of_another_shape_is_a_difference(pic):
    got = planes()
    got[2] = got[2][:, :8]
    d = H.first_difference(got, planes(), "case", pic)
    assert d == "case plane 2: shape (16, 8), expected (16, 16)"
    with pytest.raises(pytest.fail.Exception):
        H.compare_pictures([got], [planes()], "case")
    H.compare_pictures([[np.pad(a, ((0, 16), (0, 16))) for a in planes()]], [planes()], "case", crop=True)
    with pytest.raises(pytest.fail.Exception):
        H.compare_pictures([[np.pad(a, ((0, 16), (0, 16))) for a in planes()]], [planes()], "case")


def cases_of(n):
    return [(types.SimpleNamespace(pic=object(), name="c%d" % i), None) for i in range(n)]


def test_batches_fill_the_last_one_up_from_the_front():
    cases = cases_of(7)
    got = [[cases.index(c) for c in batch] for batch in H.batches_of(cases, 3)]
    assert got == [[0, 1, 2], [3, 4, 5], [6, 0, 1]]


def test_a_batch_needs_distinct_pictures():
    with pytest.raises(AssertionError):
        list(H.batches_of(cases_of(2), 3))
    cases = cases_of(3)
    cases[1] = (types.SimpleNamespace(pic=cases[0][0].pic, name="again"), None)
    with pytest.raises(AssertionError):
        list(H.batches_of(cases, 3))


class Recorder:
    """stands in for HipReconstructor: records the calls by name"""

    def __init__(self, *a, **kw):
        self.calls, self.made = [], (a, kw)

    def __getattr__(self, name):
        return lambda *a: self.calls.append((name,) + a) or "block of %s" % name

    def close(self):
        self.calls.append(("close",))


@pytest.mark.parametrize("road,want", [
    ("upload", [("upload", 3, ["pic"])]),
    ("packed", [("pack", "pic", "lib"), ("upload_packed", 3, "pic", "block of pack")]),
    ("compact", [("pack_compact", "pic", "lib"), ("upload_compact", 3, "pic", "block of pack_compact")]),
])
def test_put_makes_the_call_its_road_names(road, want):
    hip = Recorder()
    H.put(hip, "lib", 3, "pic", road)
    assert hip.calls == want


def test_an_unknown_road_raises():
    hip = Recorder()
    with pytest.raises(ValueError):
        H.put(hip, "lib", 0, "pic", "comit")
    assert hip.calls == []


def test_the_reconstructor_is_closed_when_the_body_raises(monkeypatch):
    monkeypatch.setattr(H, "HipReconstructor", Recorder)
    with pytest.raises(KeyError):
        with H.reconstructor("lib", 4, 3, slots=2) as hip:
            assert hip.made == ((4, 3), dict(lib="lib", slots=2))
            raise KeyError("in the body")
    assert hip.calls == [("close",)]


@pytest.mark.parametrize("args", ["--mbw 2 --mbh 2 --frames 2 --seed 9 --coded 30", "--mbw 2 --mbh 2 --frames 2 --seed 9 --coded 30 --cabac"], ids=["cavlc", "cabac"])
def test_write_stream_writes_what_generate_caches(tmp_path, args):
    data = synth_cases.write_stream(tmp_path, args)
    assert data == open(synth_cases.generate(args), "rb").read() and data == (tmp_path / "s.264").read_bytes()
    again, dump = synth_cases.write_stream(tmp_path, args, "t", dumps=("mv",))
    assert again == data and dump == str(tmp_path / "t.mv") and (tmp_path / "t.mv").stat().st_size > 0
