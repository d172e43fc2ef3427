"""p264hip_reconstruct decides three launch shapes from the batch alone: workgroups per picture of the motion-compensation launch,
wavefronts per workgroup of the intra launch (and whether the loop filter's edge info rides in it), and the loop filter's pictures
per workgroup / band height / odd_single / wavefronts.  The decisions are functions of the geometry, the compute units, the batch
size, what kinds of picture the batch holds and the P264AMD_* knobs - so they are pinned as a table: tests/golden/launch_shapes.json
holds p264hip_last_launch() of every case below as tests/golden/make_launch_shapes.py recorded it on an MI355X before the function
was regrouped into named steps.  The pictures' bytes are other tests' business (test_gpu_batch_shapes, test_gpu_distinct_shapes).

A case = a geometry of the suite's smallest synthetic streams, a batch size, the kinds of picture in the batch, optionally one set
of shape knobs.  Batch sizes 1 .. 1281: on 256 compute units 1 .. 6 pictures per k_deblock workgroup and all three intra_waves."""
import json
import os

import pytest

from p264decoder_amd import Parser, _native as N
from tests import synth_cases
from tests.hip_harness import reconstructor

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(synth_cases.GOLDEN, "launch_shapes.json")
SIZES = (1, 2, 255, 256, 257, 513, 769, 1025, 1281)

# geometry -> the suite's case (IDR + P pictures), and synth264 arguments of the same geometry for the other kinds of picture
GEOMETRY = {
    "tiny_1x1": "--mbw 1 --mbh 1",
    "col_Nx1": "--mbw 1 --mbh 7",
    "wide_70": "--mbw 70 --mbh 3",
    "qpdelta": "--mbw 11 --mbh 9",
}
MAIN = " --frames 4 --seed 71 --refs 2 --bframes 1 --coded 30 --maxlevel 8"           # I P B ...: the B picture
WEIGHTED = " --frames 3 --gop 0 --seed 72 --refs 2 --wp --coded 30 --maxlevel 8"      # I P P: P pictures with explicit weights
# composition -> the kinds of its pictures: entry 0 of the batch is the first kind, every other entry the last
COMPOSITION = {"I": ("I",), "P": ("P",), "IP": ("I", "P"), "B": ("B", "P"), "WP": ("WP", "P")}

K = "P264AMD_"
CASES = [(g, n, "P", {}) for g in ("qpdelta",) for n in SIZES] + [
    # 210 macroblocks: enough work-list chunks for the floor of 48 motion-compensation workgroups per picture (smaller
    # pictures stop at their max_chunks cap first)
    ("wide_70", 1, "P", {}), ("wide_70", 513, "P", {}), ("wide_70", 257, "B", {}), ("wide_70", 1025, "I", {}),
    ("col_Nx1", 1, "I", {}), ("col_Nx1", 257, "I", {}), ("col_Nx1", 1281, "I", {}), ("col_Nx1", 2, "IP", {}), ("col_Nx1", 769, "IP", {}),
    ("col_Nx1", 513, "P", {}), ("col_Nx1", 1025, "P", {}),
    ("tiny_1x1", 255, "P", {}), ("tiny_1x1", 256, "P", {}), ("tiny_1x1", 1025, "P", {}), ("tiny_1x1", 513, "B", {}), ("tiny_1x1", 257, "WP", {}),
    ("qpdelta", 1, "B", {}), ("qpdelta", 1025, "B", {}), ("qpdelta", 2, "WP", {}), ("qpdelta", 769, "WP", {}), ("qpdelta", 513, "I", {}),
    ("qpdelta", 1281, "IP", {}),
    # the knobs (read once, when the context is created); out-of-range values and knobs a batch cannot honour are ignored
    ("qpdelta", 513, "P", {K + "DEBLOCK_RB_LOG2": "3"}),
    ("qpdelta", 513, "P", {K + "DEBLOCK_RB_LOG2": "2", K + "DEBLOCK_ODD_SINGLE": "1"}),
    ("qpdelta", 769, "P", {K + "DEBLOCK_PICS_PER_WG": "5", K + "DEBLOCK_RB_LOG2": "2", K + "DEBLOCK_ODD_SINGLE": "1"}),
    ("qpdelta", 769, "P", {K + "DEBLOCK_PICS_PER_WG": "17"}),
    ("col_Nx1", 1025, "P", {K + "DEBLOCK_ODD_SINGLE": "0"}),
    ("col_Nx1", 1281, "P", {K + "DEBLOCK_RB_LOG2": "1", K + "DEBLOCK_PICS_PER_WG": "13"}),
    ("qpdelta", 1281, "P", {K + "DEBLOCK_WAVES": "2"}),
    ("qpdelta", 255, "P", {K + "BS_FUSED": "0"}),
    ("tiny_1x1", 2, "P", {K + "BS_FUSED": "3"}),
    ("qpdelta", 256, "P", {K + "BS_FUSED": "40"}),
    ("qpdelta", 513, "B", {K + "BS_FUSED": "16"}),
    ("wide_70", 256, "P", {K + "MC_WGS_PER_PIC": "7"}),
    ("wide_70", 257, "P", {K + "MC_WGS_PER_PIC": "1000"}),
    ("wide_70", 2, "P", {K + "MC_BAND_LOG2": "0"}),
    ("col_Nx1", 257, "I", {K + "INTRA_WAVES": "2"}),
    ("tiny_1x1", 1281, "WP", {K + "INTRA_WAVES": "16"}),
]


def case_id(case):
    g, n, comp, knobs = case
    return "-".join([g, str(n), comp] + ["%s=%s" % (k[len(K):], v) for k, v in sorted(knobs.items())])


_pictures = {}


def pictures(lib, geometry):
    """{kind: a parsed picture of that kind}, slots the pictures' frame stores need; parsed once per geometry"""
    if geometry not in _pictures:
        kinds, slots = {}, 0
        for spec in (geometry, GEOMETRY[geometry] + MAIN, GEOMETRY[geometry] + WEIGHTED):
            parser = Parser(quiet=True, lib=lib)
            for p in parser.parse_stream(open(synth_cases.generate(spec), "rb").read()):
                d = p.desc
                kind = "WP" if d.explicit_wp else {N.SLICE_I: "I", N.SLICE_P: "P", N.SLICE_B: "B"}[d.slice_type]
                if kind == "WP" and d.slice_type != N.SLICE_P:
                    continue
                kinds.setdefault(kind, p)
            slots = max(slots, parser.slots)
            parser.close()
        assert set(kinds) == {"I", "P", "B", "WP"}, sorted(kinds)
        _pictures[geometry] = (kinds, slots)
    return _pictures[geometry]


def run_case(lib, case, setenv):
    """The case's batch - one upload of its distinct pictures, clones for the rest, every entry on a stream of its own -
    reconstructed once and synced: p264hip_last_launch() as a dict.  setenv(name, value) sets the knobs for the context."""
    geometry, n, comp, knobs = case
    for k, v in knobs.items():
        setenv(k, v)
    kinds, slots = pictures(lib, geometry)
    distinct = [kinds[k] for k in COMPOSITION[comp]][:n]
    with reconstructor(lib, distinct[0].mb_w, distinct[0].mb_h, n_streams=n, slots=slots, max_pictures=n) as hip:
        hip.upload(0, distinct)
        for dst in range(len(distinct), n):
            hip.clone_picture(dst, len(distinct) - 1)
        hip.reconstruct(list(range(n)), list(range(n)))
        hip.sync()
        return hip.last_launch()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_the_table_is_the_recorded_one(golden):
    assert sorted(golden["cases"]) == sorted(case_id(c) for c in CASES)
    assert {c[1] for c in CASES} == set(SIZES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_launch_shapes(lib, golden, case, monkeypatch):
    for name in list(os.environ):
        if name.startswith(K + "MC_") or name.startswith(K + "DEBLOCK_") or name in (K + "INTRA_WAVES", K + "BS_FUSED"):
            monkeypatch.delenv(name)
    got = run_case(lib, case, monkeypatch.setenv)
    assert got["compute_units"] == golden["compute_units"], \
        "the table was recorded on %d compute units, this device reports %d: the shapes follow the device's size, record the table " \
        "for it (tests/golden/make_launch_shapes.py)" % (golden["compute_units"], got["compute_units"])
    assert got == golden["cases"][case_id(case)], "%s: launched %s, recorded %s" % (case_id(case), got, golden["cases"][case_id(case)])
