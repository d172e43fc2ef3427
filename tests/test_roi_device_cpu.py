"""The host side of the export from an ROI list in device memory (include/p264hip.h: p264hip_export_rois_device), no GPU: the status
rule p264hip_roi_status - the text k_roi_plan runs - against p264hip_rois_check / p264hip_rois_aa_check and against the Python model
of tests/roi_device_checker.py; the bounds of p264hip_rois_device_plan - what keeps a device-list call inside its scratch, its grid
and its LDS - against every ROI that passes the rule; the host refusals; rois_from_boxes; the two new structures; k_roi_plan in the
code object."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import roi_device_checker as DK
from tests import test_roi_cpu as T0

EINVAL = -1
MB_W, MB_H, STREAMS, SLOTS = T0.MB_W, T0.MB_H, T0.STREAMS, T0.SLOTS
FILL_WORD = T0.FILL_WORD
AA = N.FILTER_BILINEAR_AA
T_CAP = 20480                                               # P264HIP_ROI_AA_TILE_VALUES
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
OUTPUTS = [(2, 2), (6, 70), (34, 18), (162, 98), (518, 4), (224, 224)]
REDUCTIONS = [0, 1, 2, 3, 8, 32]


def desc(size=(34, 18), filter=0, fmt="rgbp", **kw):
    return N.resize_desc(fmt, size, (0, 0, 2, 2), None, filter=filter, **kw)


def c_status(lib, row, r, mb, store=(STREAMS, SLOTS), m=0):
    return lib.p264hip_roi_status(C.byref(N.Roi(*row)), C.byref(r), mb[0], mb[1], store[0], store[1], m)


def accepted(lib, row, r, mb, store=(STREAMS, SLOTS)):
    fn = lib.p264hip_rois_aa_check if r.filter == AA else lib.p264hip_rois_check
    return fn((N.Roi * 1)(N.Roi(*row)), 1, C.byref(r), FILL_WORD, mb[0], mb[1], store[0], store[1]) == 0


def drawn_rois(g, frame, size, n):
    """rows round valid ones: a valid window and rectangle (or the whole output) with 0 .. 3 members replaced by a value of a pool that
    holds the hostile ones"""
    fw, fh = frame
    W, H = size
    pool = [I32_MIN, I32_MIN + 1, I32_MAX, I32_MAX - 1, -1, -2, 0, 1, 2, 3, 4, fw, fw + 2, fh, fh - 2, W, H, W + 2, 2 ** 30, 2 ** 30 + 2, -(2 ** 30), 65536, 33 * W, 32 * W + 2]
    rows = []
    for _ in range(n):
        w, h = 2 * int(g.integers(1, fw // 2 + 1)), 2 * int(g.integers(1, fh // 2 + 1))
        if g.integers(0, 2):
            w, h = min(w, 2 * int(g.integers(1, 40))), min(h, 2 * int(g.integers(1, 40)))
        row = [int(g.integers(0, STREAMS)), int(g.integers(0, SLOTS)), 2 * int(g.integers(0, (fw - w) // 2 + 1)), 2 * int(g.integers(0, (fh - h) // 2 + 1)), w, h, 0, 0, 0, 0]
        if g.integers(0, 3):
            dw, dh = 2 * int(g.integers(1, W // 2 + 1)), 2 * int(g.integers(1, H // 2 + 1))
            row[6:] = [2 * int(g.integers(0, (W - dw) // 2 + 1)), 2 * int(g.integers(0, (H - dh) // 2 + 1)), dw, dh]
        for _ in range(int(g.integers(0, 4))):
            row[int(g.integers(0, 10))] = pool[int(g.integers(0, len(pool)))] if g.integers(0, 4) else int(g.integers(-6, 100))
        rows.append(tuple(row))
    return rows


@pytest.mark.parametrize("mb,size", [((MB_W, MB_H), (34, 18)), ((MB_W, MB_H), (2, 2)), ((120, 68), (224, 224)), ((120, 68), (6, 70))])
def test_the_status_is_the_first_refusal_of_the_checks(lib, mb, size):
    frame = (mb[0] * 16, mb[1] * 16)
    g = np.random.default_rng(2670 + size[0])
    rows = drawn_rois(g, frame, size, 6000)
    # sums that leave 32 bits: each member alone is plausible
    rows += [(0, 0, I32_MAX - 1, 0, 2, 2, 0, 0, 0, 0), (0, 0, 2, 2, I32_MAX - 1, 2, 0, 0, 0, 0), (0, 0, 0, I32_MAX - 1, 2, I32_MAX - 1, 0, 0, 0, 0),
             (0, 0, 0, 0, 2, 2, I32_MAX - 1, 0, I32_MAX - 1, 2), (0, 0, 0, 0, 2, 2, 0, 2 ** 30, 2, 2 ** 30), (0, 0, 0, 0, 2 ** 30, 2, 0, 0, 2 ** 27, 2),
             (I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN, I32_MIN), (I32_MAX,) * 10, (0, 0) + (I32_MAX - 1,) * 8]
    seen = {0: set(), AA: set()}
    for filter in (0, AA):
        r = desc(size, filter)
        for row in rows:
            st = c_status(lib, row, r, mb)
            assert st == DK.status(row, size, filter, frame, (STREAMS, SLOTS)), (row, filter)
            assert (st == 0) == accepted(lib, row, r, mb), (row, filter, st)
            seen[filter].add(st)
    assert seen[0] == {0, 2, 4, 5, 6, 7, 8, 9} and seen[AA] == {0, 2, 4, 5, 6, 7, 8, 9, 10}


def test_of_two_broken_rules_the_first_is_reported(lib):
    size, mb, frame = (34, 18), (MB_W, MB_H), (80, 48)
    base = dict(stream=0, slot=0, left=2, top=2, width=62, height=30, dst_left=2, dst_top=2, dst_width=20, dst_height=10)
    breaks = {2: dict(stream=-1), 4: dict(left=-2), 5: dict(top=3), 6: dict(height=60), 7: dict(dst_left=-2), 8: dict(dst_top=3), 9: dict(dst_height=30),
              10: dict(width=66, dst_width=2)}
    names = [k for k, _ in N.Roi._fields_]
    r = desc(size, AA)
    assert c_status(lib, [base[k] for k in names], r, mb) == 0
    for a in breaks:
        for b in breaks:
            f = dict(base)
            f.update(breaks[a])
            f.update(breaks[b])
            row = [f[k] for k in names]
            assert c_status(lib, row, r, mb) == min(a, b) == DK.status(row, size, AA, frame, (STREAMS, SLOTS)), (a, b)
    # slot 2 of 2 and slot -1 are out of range; max_reduction narrows rule 10 and nothing else; filter 0 has no rule 10
    row = [base[k] for k in names]
    assert c_status(lib, row[:1] + [SLOTS] + row[2:], r, mb) == 2 == c_status(lib, row[:1] + [-1] + row[2:], r, mb)
    for m, want in ((0, 0), (32, 0), (4, 0), (3, 10), (1, 10)):         # 62 x 30 into 20 x 10: 3.1 : 1
        assert c_status(lib, row, r, mb, m=m) == want == DK.status(row, size, AA, frame, (STREAMS, SLOTS), m), m
    assert c_status(lib, row, desc(size, 0), mb, m=1) == 0
    assert lib.p264hip_roi_status(None, C.byref(r), 5, 3, 3, 2, 0) == EINVAL and lib.p264hip_roi_status(C.byref(N.Roi(*row)), None, 5, 3, 3, 2, 0) == EINVAL


# ---- the plan: a wrong bound here is a write outside the scratch on the device
def measure(lib, r, width, height, dw, dh):
    """(segment words, tiles, bytes of dynamic LDS) of an ROI, from the host functions of the existing export"""
    roi = N.Roi(0, 0, 0, 0, width, height, 0, 0, dw, dh)
    words = lib.p264hip_roi_aa_segment_words(C.byref(roi), C.byref(r))
    ns_l, ns_c = C.c_int(), C.c_int()
    tw = lib.p264hip_roi_aa_tile_width(C.byref(roi), C.byref(r), C.byref(ns_l), C.byref(ns_c))
    assert words > 0 and tw in (8, 16, 32, 64)
    return words, -(-r.width // tw) * -(-r.height // 16), 32 * max(16 * ns_l.value, 8 * ns_c.value)


@pytest.mark.parametrize("size", OUTPUTS)
def test_the_plan_bounds_every_roi_that_passes_the_rule(lib, size):
    W, H = size
    r = desc(size, AA)
    cases = []                                              # (width, height, dw, dh, words, tiles, lds)
    if W * H <= 518 * 4:
        # every window size of the 80 x 48 frame into every rectangle size (none of the measured functions reads a position)
        roi = N.Roi(0, 0, 0, 0, 2, 2, 0, 0, 2, 2)
        words_of = lib.p264hip_roi_aa_segment_words
        for dw in range(2, W + 1, 2):
            for width in range(2, 81, 2):
                if width > 32 * dw:
                    continue
                _, tiles, lds = measure(lib, r, width, 2, dw, 2)
                roi.width, roi.dst_width = width, dw
                for dh in range(2, H + 1, 2):
                    roi.dst_height = dh
                    for height in range(2, 49, 2):
                        if height <= 32 * dh:
                            roi.height = height
                            cases.append((width, height, dw, dh, words_of(C.byref(roi), C.byref(r)), tiles, lds))
    g = np.random.default_rng(2671)
    for fw, fh in ((1920, 1088), (65520, 1088), (65520, 65520)):
        for _ in range(1500):
            dw, dh = (W, H) if g.integers(0, 3) == 0 else (2 * int(g.integers(1, W // 2 + 1)), 2 * int(g.integers(1, H // 2 + 1)))
            m = [1, 2, 3, 8, 32][int(g.integers(0, 5))]
            width = min(fw, m * dw) if g.integers(0, 2) else 2 * int(g.integers(1, min(fw, 32 * dw) // 2 + 1))
            height = min(fh, m * dh) if g.integers(0, 2) else 2 * int(g.integers(1, min(fh, 32 * dh) // 2 + 1))
            cases.append((width, height, dw, dh) + measure(lib, r, width, height, dw, dh))
    a = np.array(cases, np.int64)
    assert len(a) > 4000
    for m in REDUCTIONS:
        plan = N.rois_device_plan(r, m, lib)
        mm = m or 32
        passing = a[(a[:, 0] <= mm * a[:, 2]) & (a[:, 1] <= mm * a[:, 3])]
        assert len(passing) > 100
        for row in passing[:50]:                            # (the mask is the rule's: the model says so for whole frames that hold the window)
            assert DK.status((0, 0, 0, 0, row[0], row[1], 0, 0, row[2], row[3]), size, AA, (65520, 65520), (1, 1), m) == 0
        assert passing[:, 4].max() <= plan["seg_words"], (m, passing[passing[:, 4].argmax()], plan)
        assert passing[:, 5].max() <= plan["aa_tiles"], (m, plan)
        assert passing[:, 6].max() <= plan["aa_lds_bytes"] <= 2 * T_CAP, (m, passing[passing[:, 6].argmax()], plan)
        assert plan["rois_per_pair"] == (N.ROI_SCRATCH_BYTES // 4) // plan["seg_words"] >= 1
        # the bound is not slack: the widest window of the whole output reaches it, in a frame that holds it
        reach = (0, 0, 0, 0, mm * W, mm * H, 0, 0, 0, 0)
        assert lib.p264hip_roi_status(C.byref(N.Roi(*reach)), C.byref(r), 4095, 4095, 1, 1, m) == 0
        words, tiles, lds = measure(lib, r, mm * W, mm * H, W, H)
        assert words == plan["seg_words"] and tiles == plan["aa_tiles"] and lds <= plan["aa_lds_bytes"]
    # filter 0: a word per entry of the whole output, no tiles of its own
    pad4 = lambda n: (n + 3) & ~3
    plan = N.rois_device_plan(desc(size, 0), 0, lib)
    assert plan == dict(seg_words=pad4(W) + pad4(H) + pad4(W // 2) + pad4(H // 2), rois_per_pair=(N.ROI_SCRATCH_BYTES // 4) // plan["seg_words"], aa_tiles=0, aa_lds_bytes=0)


def test_the_plan_at_the_largest_outputs_and_its_refusals(lib):
    """16384 samples a side: the window stops at the frame's 65534, and a pair still holds an ROI; 224 x 224 at 32:1 is the header's 89 KB"""
    for size in ((16384, 16384), (16384, 2), (2, 16384), (4096, 4096)):
        for m in (0, 3):
            plan = N.rois_device_plan(desc(size, AA), m, lib)
            assert plan["rois_per_pair"] >= 1 and plan["seg_words"] <= 300000 and plan["aa_lds_bytes"] <= 2 * T_CAP
            r = desc(size, AA)
            mm = m or 32
            for dw in (size[0], size[0] // 2 & ~1 or 2, 2048 if size[0] >= 2048 else 2):
                words, tiles, lds = measure(lib, r, min(65534, mm * dw), min(65534, mm * size[1]), dw, size[1])
                assert words <= plan["seg_words"] and tiles <= plan["aa_tiles"] and lds <= plan["aa_lds_bytes"]
    plan = N.rois_device_plan(desc((224, 224), AA), 0, lib)
    assert 88000 < 4 * plan["seg_words"] < 90000 and plan["rois_per_pair"] in (188, 189)
    # an axis of D samples at m:1 is D words and D rows of 2 m weights: 1 + m words a sample, so 4:1 costs 5 / 33 of 32:1
    assert 33 * N.rois_device_plan(desc((224, 224), AA), 4, lib)["seg_words"] == 5 * plan["seg_words"]
    out = N.RoisPlan()
    for r, m in ((desc((34, 18), 0), 1), (desc((34, 18), 0), -1), (desc((34, 18), AA), 33), (desc((34, 18), AA), -1), (desc((33, 18), AA), 0), (desc((34, 18), 1), 0),
                 (desc((34, 18), 0, "i420", dtype="f16"), 0)):
        assert lib.p264hip_rois_device_plan(C.byref(r), m, C.byref(out)) == EINVAL
    assert lib.p264hip_rois_device_plan(None, 0, C.byref(out)) == EINVAL and lib.p264hip_rois_device_plan(C.byref(desc()), 0, None) == EINVAL


def test_the_host_refusals_of_a_device_list(lib):
    table = (C.c_int32 * STREAMS)(0, -1, 1)

    def check(r=None, fill=FILL_WORD, mb=(MB_W, MB_H), store=(STREAMS, SLOTS), null=False, **kw):
        f = dict(rois_dev=0x7f0000001000, count_dev=None, status_dev=None, slot_of_stream=None, after_stream=None, before_stream=None, n=5, max_reduction=0, flags=0)
        f.update(kw)
        l = N.RoisDev(*[f[k] for k, _ in N.RoisDev._fields_])
        return lib.p264hip_rois_device_check(None if null else C.byref(l), C.byref(r) if r is not None else None, fill, mb[0], mb[1], store[0], store[1])
    for filter in (0, AA):                                  # one accepted description per filter, with everything a list may carry
        assert check(desc(filter=filter)) == 0
        assert check(desc(filter=filter, fmt="rgb24", dtype="f16", scale=1 / 255), slot_of_stream=table, count_dev=0x1000, status_dev=0x2000, flags=3, after_stream=0x10,
                     max_reduction=8 if filter else 0, n=1 << 20) == 0
    refused = [
        lambda: check(None), lambda: check(desc(), null=True),
        # what p264hip_rois_frame_bytes / _aa_frame_bytes refuses in the description
        lambda: check(desc(filter=1)), lambda: check(desc(fmt=4)), lambda: check(desc(size=(33, 18))), lambda: check(desc(size=(16386, 2))), lambda: check(desc(fmt="i420", dtype="f32")),
        lambda: check(desc(scale=1.0)), lambda: check(desc(pitch=32)), lambda: check(desc(filter=AA, matrix=2)), lambda: check(desc(frame_stride=3 * 34 * 18 - 1)),
        # the list
        lambda: check(desc(), rois_dev=None), lambda: check(desc(), rois_dev=0x7f0000001004), lambda: check(desc(), rois_dev=0x7f0000001001), lambda: check(desc(), n=0), lambda: check(desc(), n=-1),
        lambda: check(desc(), fill=FILL_WORD | 1 << 24), lambda: check(desc(), mb=(4096, 3)), lambda: check(desc(), mb=(5, 4096)), lambda: check(desc(), mb=(0, 3)),
        lambda: check(desc(), store=(0, 2)), lambda: check(desc(), store=(3, 0)),
        lambda: check(desc(), max_reduction=1), lambda: check(desc(filter=AA), max_reduction=33), lambda: check(desc(filter=AA), max_reduction=-1),
        lambda: check(desc(), flags=4), lambda: check(desc(), flags=-1),
        lambda: check(desc(), slot_of_stream=(C.c_int32 * STREAMS)(0, SLOTS, 0)), lambda: check(desc(), slot_of_stream=(C.c_int32 * STREAMS)(0, 0, -2)),
    ]
    for i, f in enumerate(refused):
        assert f() == EINVAL, "refusal %d" % i
    assert check(desc(), mb=(4095, 4095)) == 0              # 65520 samples a side


# ---- rois_from_boxes
def plain_rois(boxes, streams, slots, frame, letterbox_to=None):
    """the rows, box by box in plain Python from the words of rois_from_boxes' description"""
    fw, fh = frame
    rows = []
    for (x1, y1, x2, y2), s, k in zip(boxes, streams, slots):
        row = [s, k, 0, 0, 0, 0, 0, 0, 0, 0]
        if all(math.isfinite(v) for v in (x1, y1, x2, y2)):
            x1, x2 = (min(max(v, 0), fw) for v in (x1, x2))
            y1, y2 = (min(max(v, 0), fh) for v in (y1, y2))
            if x2 > x1 and y2 > y1:
                left, top = 2 * math.floor(x1 / 2), 2 * math.floor(y1 / 2)
                row[2:6] = [left, top, 2 * math.ceil(x2 / 2) - left, 2 * math.ceil(y2 / 2) - top]
                if letterbox_to:
                    row[6:] = N.letterbox(row[4], row[5], *letterbox_to)
        rows.append(row)
    return rows


def test_rois_from_boxes_on_cpu_tensors(lib):
    torch = pytest.importorskip("torch")
    from p264decoder_amd.rois import rois_from_boxes
    g = np.random.default_rng(2672)
    frame = (1920, 1088)
    n = 600
    b = g.uniform(-200, 2000, (n, 4))
    b[:, 1] = g.uniform(-100, 1150, n)
    b[:, 2:] = b[:, :2] + g.uniform(-50, 900, (n, 2))       # (some reversed, some outside)
    inf, nan = float("inf"), float("nan")
    special = [(5, 5, 6, 6), (5.5, 7.25, 5.75, 7.5), (0, 0, 1920, 1088), (-50, -50, 5000, 5000), (1919, 1087, 1920, 1088), (1920, 0, 2000, 10), (-10, 5, 0, 9), (3, 3, 3, 9), (9, 3, 3, 9),
               (nan, 0, 10, 10), (0, 0, inf, 10), (-inf, 0, 10, 10), (0, nan, 10, nan), (1e30, 1e30, 2e30, 2e30), (-1e30, -1e30, 1e30, 1e30), (4, 4, 6, 6), (4.0001, 4, 5.9999, 6.0001)]
    b[:len(special)] = special
    streams, slots = g.integers(0, 7, n), g.integers(0, 2, n)
    for dtype in (torch.float32, torch.float64, torch.int64, torch.int32):
        bb = np.nan_to_num(np.clip(b, -1e9, 1e9)).round() if dtype in (torch.int64, torch.int32) else b
        t = torch.tensor(bb, dtype=dtype)
        boxes = t.tolist()                                  # (what the tensor holds: float32 has rounded the drawn numbers)
        for lb in (None, (224, 224), (640, 360), (2, 50)):
            got = rois_from_boxes(t, torch.tensor(streams), torch.tensor(slots), frame, lb)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, 10)
            want = plain_rois(boxes, streams.tolist(), slots.tolist(), frame, lb)
            assert got.tolist() == want, (dtype, lb)
            size = lb or (224, 224)
            empty = 0
            for row in want:
                st = DK.status(row, size, 0, frame, (7, 2))
                assert st == 0 or (row[2:6] == [0, 0, 0, 0] and st == DK.WINDOW_EMPTY), row
                assert st != 0 or (row[4] >= 2 and row[5] >= 2)
                empty += st != 0
            assert 10 < empty < n - 100                     # (the draw holds both kinds)
    one = rois_from_boxes(torch.tensor([[5.0, 5.0, 6.0, 6.0]]), 3, -1, frame)
    assert one.tolist() == [[3, -1, 4, 4, 2, 2, 0, 0, 0, 0]]
    with pytest.raises(ValueError):
        rois_from_boxes(torch.zeros(3, 5), 0, 0, frame)


def test_abi_mirror_of_the_two_structures(lib):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "p264hip.h"
#define O(f) offsetof(p264hip_rois_dev_t, f)
int main(void) {
  printf("plan %zu %zu %zu %zu %zu\n", sizeof(p264hip_rois_plan_t), offsetof(p264hip_rois_plan_t, seg_words), offsetof(p264hip_rois_plan_t, rois_per_pair),
         offsetof(p264hip_rois_plan_t, aa_tiles), offsetof(p264hip_rois_plan_t, aa_lds_bytes));
  printf("list %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(p264hip_rois_dev_t), O(rois_dev), O(count_dev), O(status_dev), O(slot_of_stream), O(after_stream), O(before_stream),
         O(n), O(max_reduction), O(flags));
  printf("codes %d %d %d %d %d %d %d %d %d %d %d %d %d\n", P264HIP_ROI_OK, P264HIP_ROI_UNUSED, P264HIP_ROI_BAD_PICTURE, P264HIP_ROI_NO_PICTURE, P264HIP_ROI_WINDOW_EMPTY,
         P264HIP_ROI_WINDOW_ODD, P264HIP_ROI_WINDOW_OUTSIDE, P264HIP_ROI_RECT_SMALL, P264HIP_ROI_RECT_ODD, P264HIP_ROI_RECT_OUTSIDE, P264HIP_ROI_REDUCTION,
         P264HIP_ROIS_AFTER, P264HIP_ROIS_BEFORE);
  return 0; }
'''
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.run(["gcc", "-I" + inc, c, "-o", exe], check=True)
        out = dict((l.split()[0], [int(x) for x in l.split()[1:]]) for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())
    P, L = N.RoisPlan, N.RoisDev
    assert out["plan"] == [C.sizeof(P), P.seg_words.offset, P.rois_per_pair.offset, P.aa_tiles.offset, P.aa_lds_bytes.offset] == [16, 0, 4, 8, 12]
    assert out["list"] == [C.sizeof(L)] + [getattr(L, k).offset for k, _ in L._fields_]
    assert out["codes"] == [N.ROI_OK, N.ROI_UNUSED, N.ROI_BAD_PICTURE, N.ROI_NO_PICTURE, N.ROI_WINDOW_EMPTY, N.ROI_WINDOW_ODD, N.ROI_WINDOW_OUTSIDE, N.ROI_RECT_SMALL,
                            N.ROI_RECT_ODD, N.ROI_RECT_OUTSIDE, N.ROI_REDUCTION, N.ROIS_AFTER, N.ROIS_BEFORE] == list(range(11)) + [1, 2]
    assert [getattr(DK, k) for k in ("OK", "UNUSED", "BAD_PICTURE", "NO_PICTURE", "WINDOW_EMPTY", "WINDOW_ODD", "WINDOW_OUTSIDE", "RECT_SMALL", "RECT_ODD", "RECT_OUTSIDE", "REDUCTION")] == list(range(11))
    for f in ("p264hip_roi_status", "p264hip_rois_device_plan", "p264hip_rois_device_check", "p264hip_export_rois_device", "p264pipe_export_last_rois_device"):
        assert hasattr(lib, f), f


def test_k_roi_plan_is_in_the_code_object_without_spills_or_scratch(lib):
    from p264decoder_amd.tools import kernel_resources as kr
    try:
        res = kr.kernel_resources(N.LIB_PATH)
    except RuntimeError as e:
        pytest.skip(str(e))
    assert "k_roi_plan" in res, sorted(res)
    r = res["k_roi_plan"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, r
