"""The launch plan (csrc/hip/launch_plan.h) on the CPU: plan_launches() is plain C++ - a function of geometry, compute units, batch
size, the kinds of picture in the batch and the P264AMD_* knobs - so a small program built with g++ runs it without HIP and
without a GPU.  Three things are asserted: the 47 cases an MI355X recorded (tests/golden/launch_shapes.json, the table of
test_gpu_launch_shapes) come out as recorded; every combination of kinds gets the kernel instances the rules below name, with
the invariants that tie the stages together; knob values out of range are ignored.

The program reads one case per line, `mb_w mb_h n compute_units  i p b wp dup t8 i8 sc cr  [P264AMD_NAME=value ...]` (sc, cr: how many
pictures take the scaled road / have a Cr QP offset of their own), feeds the
knobs through launch_knobs_read by a getenv of its own and prints `key=value ...`: the plan's enums, copy_scale_table, the
band of the work lists, every field of the plan's p264hip_launch_info_t, and the work lists' layout (max_chunks per pass and list, the
chunk sizes and key counts of launch_shared.h: tests/test_worklist_cpu.py reads them through this program too)."""
import itertools
import json
import os
import subprocess
import tempfile

import pytest

from tests.batch_kinds import plan_rules
from tests.test_gpu_launch_shapes import CASES, COMPOSITION, GEOMETRY, GOLDEN, K, case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "launch_plan.h"
int main(void) {
    static const char *sort[] = { "none", "plain", "wp", "b", "b_wp", "scaled", "scaled_p" }, *mc[] = { "none", "plain", "wp" };
    static const char *residual[] = { "none", "t8x8", "scaled_inter" }, *edge[] = { "fused", "bs_false", "bs_true" };
    static const char *intra[] = { "dense", "sparse", "dense_i8", "sparse_i8", "dense_scaled", "sparse_scaled" };
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int mb_w, mb_h, n, cu, f[7], cr;
        BatchKinds k;
        in >> mb_w >> mb_h >> n >> cu >> f[0] >> f[1] >> f[2] >> f[3] >> f[4] >> f[5] >> f[6] >> k.sc >> cr;
        if (!in) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        k.i = f[0]; k.p = f[1]; k.b = f[2]; k.wp = f[3]; k.dup = f[4]; k.t8 = f[5]; k.i8 = f[6]; k.cr = cr != 0; k.n_cr = cr;
        std::map<std::string, std::string> env;
        for (std::string kv; in >> kv; ) env[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
        const LaunchKnobs knobs = launch_knobs_read([&](const char *name) { auto it = env.find(name); return it == env.end() ? (const char *)nullptr : it->second.c_str(); });
        const LaunchDevice dev = launch_device(mb_w, mb_h, cu, knobs);
        const LaunchPlan pl = plan_launches(dev, knobs, k, n);
        const p264hip_launch_info_t &li = pl.info;
        printf("sort=%s mc=%s second=%d residual=%s intra=%s edge=%s copy_scale_table=%d band_log2=%u n_bands=%u "
               "pictures=%d compute_units=%d mc_wgs_per_picture=%d intra_waves=%d edge_info_fused=%d deblock_pics_per_wg=%d deblock_rb_log2=%d "
               "deblock_waves=%d deblock_wgs=%d deblock_odd_single=%d t8x8_wgs=%d scaled_pictures=%d intra_i8=%d deblock_cr=%d cr_pictures=%d",
               sort[(int)pl.sort], mc[(int)pl.mc], (int)pl.mc_second, residual[(int)pl.residual], intra[(int)pl.intra], edge[(int)pl.edge], (int)pl.copy_scale_table,
               dev.ml.band_log2, dev.ml.n_bands, li.pictures, li.compute_units, li.mc_wgs_per_picture, li.intra_waves, li.edge_info_fused, li.deblock_pics_per_wg,
               li.deblock_rb_log2, li.deblock_waves, li.deblock_wgs, li.deblock_odd_single, li.t8x8_wgs, li.scaled_pictures, li.intra_i8, (int)pl.deblock_cr, li.cr_pictures);
        // the work lists' layout and the constants tests/worklist_model.py types in: [pass * ML_LISTS + list]
        for (int l = 0; l < 2 * ML_LISTS; l++) printf(" max_chunks%d=%u", l, dev.ml.max_chunks[l]);
        for (int l = 0; l < ML_LISTS; l++) printf(" chunk_items%d=%d list_keys%d=%d", l, mc_chunk_items(l), l, mc_list_keys(l));
        printf(" MCY_KEYS=%d MCC_KEYS=%d MC_MAX_BANDS=%d ML_LISTS=%d ML_YM=%d ML_YQ=%d ML_CM=%d ML_CQ=%d\n", MCY_KEYS, MCC_KEYS, MC_MAX_BANDS, ML_LISTS,
               (int)ML_YM, (int)ML_YQ, (int)ML_CM, (int)ML_CQ);
    }
    return 0;
}
'''

KINDS = ("i", "p", "b", "wp", "dup", "t8", "i8", "sc", "cr")
MB = {"tiny_1x1": (1, 1), "col_Nx1": (1, 7), "wide_70": (70, 3), "qpdelta": (11, 9)}     # macroblocks: GEOMETRY's --mbw / --mbh
CU = 256                                                                                 # what the golden table was recorded on


@pytest.fixture(scope="module")
def plan():
    """plan(cases) -> one dict per case; a case = (mb_w, mb_h, n, compute_units, {kind: value}, {knob: value})"""
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(src, "w").write(SRC)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "p264decoder_amd", "csrc", "hip"), src, "-o", exe], check=True)

        def run(cases):
            text = "".join("%d %d %d %d %s %s\n" % (w, h, n, cu, " ".join(str(int(kinds.get(k, 0))) for k in KINDS),
                                                  " ".join("%s=%s" % kv for kv in sorted(knobs.items())))
                           for w, h, n, cu, kinds, knobs in cases)
            r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stdout
            out = [{k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (kv.split("=") for kv in line.split())} for line in r.stdout.splitlines()]
            assert len(out) == len(cases)
            return out
        yield run


def kinds_of(comp, n):
    """what batch_fill finds in the batch of a test_gpu_launch_shapes case: entry 0 is the composition's first kind, every other
    entry its last ("B" at n = 1: a lone B picture)"""
    held = set(([COMPOSITION[comp][0]] + [COMPOSITION[comp][-1]] * (n - 1)))
    return {"i": "I" in held, "p": bool(held - {"I"}), "b": "B" in held, "wp": "WP" in held}


def test_geometry_table_is_the_gpu_test_s():
    assert {g: "--mbw %d --mbh %d" % wh for g, wh in MB.items()} == GEOMETRY


def test_the_recorded_launch_shapes(plan):
    golden = json.load(open(GOLDEN))
    assert golden["compute_units"] == CU and len(CASES) == 47 and sorted(golden["cases"]) == sorted(case_id(c) for c in CASES)
    got = plan([MB[g] + (n, CU, kinds_of(comp, n), knobs) for g, n, comp, knobs in CASES])
    wrong = {}
    for case, plan_of in zip(CASES, got):
        want = golden["cases"][case_id(case)]
        if {k: plan_of[k] for k in want} != want:
            wrong[case_id(case)] = ({k: plan_of[k] for k in want}, want)
    assert not wrong, "planned, recorded: %s" % wrong


# ---- the instance of every stage by the batch's kinds, restated from the rules (not from the header's code) ----
N_MB = 11 * 9


def expected(k, n, bs_knob):
    """tests/batch_kinds.py: plan_rules, which the batches of tests/test_gpu_batch_kinds.py are planned with too"""
    return plan_rules(k, n, bs_knob, N_MB)


def test_every_combination_of_kinds(plan):
    cases, meta = [], []
    for n in (1, 2, 257):
        for flags in itertools.product((False, True), repeat=7):
            for sc in sorted({0, 1, n}):
                for cr in sorted({0, 1, sc} if sc else {0}):             # (batch_fill counts a picture with a Cr delta as a scaled one: cr <= sc)
                    k = dict(zip(KINDS, flags + (sc, cr)))
                    if not (k["i"] or k["p"]) or (k["b"] and not k["p"]):
                        continue
                    for bs_knob in (None, 0, 3):
                        cases.append((11, 9, n, CU, k, {} if bs_knob is None else {K + "BS_FUSED": str(bs_knob)}))
                        meta.append((k, n, bs_knob))
    # (with p: six free kinds; without: i, and no b) x (sc, cr) values per n (sc 0: cr 0; sc 1: cr 0, 1; sc n > 1: cr 0, 1, n) x knob
    assert len(cases) == (64 + 16) * (3 + 6 + 6) * 3
    for (k, n, bs_knob), got in zip(meta, plan(cases)):
        what = "%s n=%d BS_FUSED=%s: %s" % (k, n, bs_knob, got)
        want = expected(k, n, bs_knob)
        assert {x: got[x] for x in want} == want, what
        assert (got["mc_wgs_per_picture"] > 0) == k["p"], what
        # the invariants across stages
        assert (got["edge_info_fused"] > 0) == (got["intra"] == "sparse" and got["edge"] == "fused"), what
        assert (got["edge"] == "bs_true") == (k["b"] or k["wp"] or k["dup"]), what
        assert (got["t8x8_wgs"] > 0) == (got["residual"] == "t8x8"), what
        assert (got["residual"] == "scaled_inter") == bool(k["sc"] and k["p"]), what
        if not k["p"]:
            assert (got["sort"], got["mc"], got["second"], got["residual"]) == ("none", "none", 0, "none"), what
        assert got["copy_scale_table"] == int(bool(k["sc"])), what
        # the Cr instances of the loop filter: with any Cr delta, and then never behind the fused edge info (such a batch is a scaled one)
        assert got["deblock_cr"] == int(bool(k["cr"])) and got["cr_pictures"] == k["cr"], what
        assert not (got["deblock_cr"] and got["edge"] == "fused"), what


def test_knob_values_out_of_range_are_ignored(plan):
    P = {"p": True}

    def one(geometry, n, knobs):
        return plan([MB[geometry] + (n, CU, P, {K + name: v for name, v in knobs.items()})])[0]
    # clamped where it is read, then used
    assert one("qpdelta", 256, {"BS_FUSED": "40"})["edge_info_fused"] == 16
    assert one("qpdelta", 256, {"BS_FUSED": "-7"})["edge_info_fused"] == 1
    # out of range where they are applied: the batch's own shape
    assert one("qpdelta", 769, {"DEBLOCK_PICS_PER_WG": "17"}) == one("qpdelta", 769, {})
    assert one("qpdelta", 769, {"DEBLOCK_PICS_PER_WG": "16"})["deblock_pics_per_wg"] == 16
    assert one("wide_70", 257, {"MC_WGS_PER_PIC": "1000"}) == one("wide_70", 257, {})
    assert one("wide_70", 257, {"MC_WGS_PER_PIC": "3"}) == one("wide_70", 257, {})
    assert one("wide_70", 256, {"MC_WGS_PER_PIC": "7"})["mc_wgs_per_picture"] == 7
    assert one("qpdelta", 513, {"DEBLOCK_RB_LOG2": "4"}) == one("qpdelta", 513, {})
    assert one("col_Nx1", 257, {"INTRA_WAVES": "17"}) == one("col_Nx1", 257, {})
    # the band of the work lists: 0 .. 9 macroblock-row exponents are taken, anything else is the built-in 16 rows
    unset = one("wide_70", 2, {})
    assert (unset["band_log2"], unset["n_bands"]) == (4, 1)
    zero = one("wide_70", 2, {"MC_BAND_LOG2": "0"})
    assert (zero["band_log2"], zero["n_bands"]) == (0, 3)
    assert one("wide_70", 2, {"MC_BAND_LOG2": "-1"}) == unset and one("wide_70", 2, {"MC_BAND_LOG2": "10"}) == unset
    # ... and the band doubles until the picture has at most MC_MAX_BANDS (32) of them: 32 rows are 32 bands of one, 33 rows 17 bands of two
    deep = plan([(8, 32, 2, CU, P, {K + "MC_BAND_LOG2": "0"}), (8, 33, 2, CU, P, {K + "MC_BAND_LOG2": "0"}), (8, 512, 2, CU, P, {})])
    assert [(d["band_log2"], d["n_bands"]) for d in deep] == [(0, 32), (1, 17), (4, 32)]
    # DEBLOCK_ODD_SINGLE is a switch: any value but 0 is "on"
    assert one("qpdelta", 769, {"DEBLOCK_ODD_SINGLE": "5"}) == one("qpdelta", 769, {"DEBLOCK_ODD_SINGLE": "1"})
