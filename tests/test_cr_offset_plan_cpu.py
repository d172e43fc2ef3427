"""The launch plan (csrc/hip/launch_plan.h) of batches that hold a picture whose Cr has a QP offset of its own, on the CPU: a g++
program of its own, like the one of tests/test_launch_plan_cpu.py, that also reads BatchKinds::cr.  With cr set (sc >= 1 then:
batch_fill counts such a picture as a scaled one) the plan selects the Cr instances of the loop filter, never the fused edge road,
and the scaled instances of sort, residual and intra; with cr clear the plan is, field for field, the plan of a BatchKinds that
never mentions it."""
import itertools
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <iostream>
#include <sstream>
#include <string>
#include "launch_plan.h"
static void show(const LaunchPlan &pl, const LaunchDevice &dev) {
    static const char *sort[] = { "none", "plain", "wp", "b", "b_wp", "scaled", "scaled_p" }, *mc[] = { "none", "plain", "wp" };
    static const char *residual[] = { "none", "t8x8", "scaled_inter" }, *edge[] = { "fused", "bs_false", "bs_true" };
    static const char *intra[] = { "dense", "sparse", "dense_i8", "sparse_i8", "dense_scaled", "sparse_scaled" };
    const p264hip_launch_info_t &li = pl.info;
    printf("sort=%s mc=%s second=%d residual=%s intra=%s edge=%s copy_scale_table=%d deblock_cr=%d band_log2=%u "
           "pictures=%d compute_units=%d mc_wgs_per_picture=%d intra_waves=%d edge_info_fused=%d deblock_pics_per_wg=%d deblock_rb_log2=%d "
           "deblock_waves=%d deblock_wgs=%d deblock_odd_single=%d t8x8_wgs=%d scaled_pictures=%d cr_pictures=%d reserved=%d,%d intra_i8=%d "
           "shapes=%u,%u,%u/%u,%u,%u/%u,%u,%u/%u,%u,%u/%u,%u,%u/%u,%u,%u mc_wgs_total=%d mc_inv_wgs=%u",
           sort[(int)pl.sort], mc[(int)pl.mc], (int)pl.mc_second, residual[(int)pl.residual], intra[(int)pl.intra], edge[(int)pl.edge], (int)pl.copy_scale_table,
           (int)pl.deblock_cr, dev.ml.band_log2, li.pictures, li.compute_units, li.mc_wgs_per_picture, li.intra_waves, li.edge_info_fused, li.deblock_pics_per_wg,
           li.deblock_rb_log2, li.deblock_waves, li.deblock_wgs, li.deblock_odd_single, li.t8x8_wgs, li.scaled_pictures, li.cr_pictures, li.reserved[0], li.reserved[1], li.intra_i8,
           pl.sort_shape.grid_x, pl.sort_shape.grid_y, pl.sort_shape.threads, pl.mc_shape.grid_x, pl.mc_shape.grid_y, pl.mc_shape.threads,
           pl.residual_shape.grid_x, pl.residual_shape.grid_y, pl.residual_shape.threads, pl.intra_shape.grid_x, pl.intra_shape.grid_y, pl.intra_shape.threads,
           pl.edge_shape.grid_x, pl.edge_shape.grid_y, pl.edge_shape.threads, pl.deblock_shape.grid_x, pl.deblock_shape.grid_y, pl.deblock_shape.threads,
           pl.mc_wgs_total, pl.mc_inv_wgs);
}
int main(void) {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int mb_w, mb_h, n, cu, f[7], sc, cr, n_cr, mention;
        in >> mb_w >> mb_h >> n >> cu >> f[0] >> f[1] >> f[2] >> f[3] >> f[4] >> f[5] >> f[6] >> sc >> cr >> n_cr >> mention;
        if (!in) { fprintf(stderr, "bad case: %s\n", line.c_str()); return 2; }
        BatchKinds k;
        k.i = f[0]; k.p = f[1]; k.b = f[2]; k.wp = f[3]; k.dup = f[4]; k.t8 = f[5]; k.i8 = f[6]; k.sc = sc;
        if (mention) { k.cr = cr != 0; k.n_cr = n_cr; }              // (mention = 0: a BatchKinds that never mentions the two)
        const LaunchKnobs knobs;
        const LaunchDevice dev = launch_device(mb_w, mb_h, cu, knobs);
        show(plan_launches(dev, knobs, k, n), dev);
        printf("\n");
    }
    return 0;
}
'''

KINDS = ("i", "p", "b", "wp", "dup", "t8", "i8")


@pytest.fixture(scope="module")
def plan():
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
        open(src, "w").write(SRC)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "p264decoder_amd", "csrc", "hip"), src, "-o", exe], check=True)

        def run(cases):
            """case: (mb_w, mb_h, n, {kind: bool}, sc, cr, n_cr, mention)"""
            text = "".join("%d %d %d 256 %s %d %d %d %d\n" % (w, h, n, " ".join(str(int(kinds.get(k, 0))) for k in KINDS), sc, cr, n_cr, mention)
                           for w, h, n, kinds, sc, cr, n_cr, mention in cases)
            r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, text=True)
            assert r.returncode == 0, r.stdout
            lines = r.stdout.splitlines()
            assert len(lines) == len(cases)
            return lines, [dict(kv.split("=") for kv in line.split()) for line in lines]
        yield run


def combinations():
    """what batch_fill can produce: wp, dup and t8 come with p, b with p"""
    for bits in itertools.product((0, 1), repeat=len(KINDS)):
        k = dict(zip(KINDS, bits))
        if not (k["i"] or k["p"]) or ((k["b"] or k["wp"] or k["dup"] or k["t8"]) and not k["p"]):
            continue
        yield k


@pytest.mark.parametrize("geometry,n", [((11, 9), 1), ((11, 9), 5), ((120, 68), 2048), ((70, 3), 300)])
def test_every_combination_of_kinds_with_a_cr_picture(plan, geometry, n):
    kinds = list(combinations())
    assert len(kinds) > 30
    n_cr = 1 + n // 3
    lines, got = plan([geometry + (n, k, max(n_cr, 1 + n // 2), 1, n_cr, 1) for k in kinds])
    _, without = plan([geometry + (n, k, max(n_cr, 1 + n // 2), 0, 0, 1) for k in kinds])
    for k, g, w in zip(kinds, got, without):
        assert g["deblock_cr"] == "1" and int(g["cr_pictures"]) == n_cr and g["reserved"] == "0,0", (k, g)
        assert g["edge"] == ("bs_true" if k["b"] or k["wp"] or k["dup"] else "bs_false") and g["edge_info_fused"] == "0", (k, g)
        assert g["intra"] == ("dense_scaled" if k["i"] else "sparse_scaled"), (k, g)
        assert g["copy_scale_table"] == "1" and int(g["scaled_pictures"]) == max(n_cr, 1 + n // 2)
        if k["p"]:
            assert g["sort"] == ("scaled" if k["b"] or k["wp"] else "scaled_p") and g["residual"] == "scaled_inter" and g["t8x8_wgs"] == "0", (k, g)
        else:
            assert (g["sort"], g["mc"], g["residual"]) == ("none", "none", "none"), (k, g)
        # the Cr instances take the roads and shapes of the same scaled batch without a delta
        assert {x: v for x, v in g.items() if x not in ("deblock_cr", "cr_pictures")} == {x: v for x, v in w.items() if x not in ("deblock_cr", "cr_pictures")}, k


@pytest.mark.parametrize("geometry,n", [((11, 9), 3), ((120, 68), 2048)])
def test_with_cr_clear_the_plan_is_the_plan_of_before(plan, geometry, n):
    kinds = list(combinations())
    for sc in (0, 2):
        a, got = plan([geometry + (n, k, sc, 0, 0, 1) for k in kinds])
        b, _ = plan([geometry + (n, k, sc, 0, 0, 0) for k in kinds])
        assert a == b
        assert all(g["deblock_cr"] == "0" and g["cr_pictures"] == "0" for g in got)
    # a plain batch of P pictures still takes the fused edge road
    _, (g,) = plan([geometry + (n, {"p": 1}, 0, 0, 0, 1)])
    assert g["edge"] == "fused" and g["intra"] == "sparse" and g["sort"] == "plain"
