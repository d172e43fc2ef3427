#!/usr/bin/env python3
"""Rate of the export of per-picture windows (p264hip_export_rois) out of a store of 1080p frames, beside the roads that existed before
it.  The roads of a case alternate repetition by repetition in one run; every repetition is closed by a sync; the median of --reps is
reported with min and max.  Bytes are counted from the shapes.  This is NOT bench.py's metric (the reconstruction); it is the figure
DESIGN.md quotes for K6b.

  a  the same work as the existing road: one ROI per frame, the whole 1920 x 1080 window to 224 x 224 planar RGB float32 normalised,
     beside p264hip_export_resized of the same description.  What the device-made taps, the per-picture segment and the per-sample
     select cost: the ROI road is required to reach 0.9 of export_resized's rate in the same run.
  b  what the feature is for: 4096 drawn windows (seeded, 64 .. 512 samples a side, two per frame) to 224 x 224 planar RGB float32 in
     ONE export_rois call, beside one export_resized call per window, measured on the first 256 of them.
  c  letterbox: every frame into 640 x 640 planar RGB float16 through letterbox(), beside export_resized to 640 x 360 followed by
     torch.nn.functional.pad on the device.

--aa-out measures the ANTIALIASED filter (p264hip_export_rois_aa, kernel_roi_aa.h) as well: the same three shapes, each beside the same
call with filter 0 from this build (what the antialiasing costs) and, for the whole frames of case a, beside
export_resized(filter="bilinear_aa") at the same shape - the kernel the ROI kernels share their passes with, so the ratio is what the
per-ROI tables, the clipping and the device-made taps cost.  No figure is required of these; DESIGN.md K6c quotes them.

--device-out measures the ROI LIST IN DEVICE MEMORY (p264hip_export_rois_device, kernel_roi_dev.h) on case b's 4096 windows: filter 0
host list against device list, filter 2 host list against device list with max_reduction 0 and 3 (the windows reduce by 2.3:1 at
most), and - what a caller whose boxes are a device tensor had to do before - .cpu(), a Python loop over the rows and the host-list
call.  Per road: the rate with a sync behind every call, the launch pairs, the scratch bytes of a pair, and the wall time until the
call RETURNS with nothing waited for (the host cost).  No figure is required of these; DESIGN.md K6d quotes them.

  python -m p264decoder_amd.tools.roi_bench [--frames 2048] [--reps 20] [--warmup 3] [--out profiles/roi_bench.json]
                                            [--aa-out profiles/roi_aa_bench.json [--only-aa]] [--device-out profiles/roi_device_bench.json [--only-device]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from p264decoder_amd.tools.resize_bench import H, MB_H, MB_W, MEAN, STD, W, alternating, entry      # noqa: E402

PER_CALL = 256              # windows of case b the one-call-per-window road is measured on


def launch_pairs(lib, rois, size):
    """how many pairs of launches p264hip_export_rois_aa makes for these ROIs (p264hip.hip: a pair ends where the next segment would
    cross P264HIP_ROI_SCRATCH_BYTES), and the words of all segments"""
    import ctypes as C
    from p264decoder_amd import _native as N
    r = N.resize_desc("rgbp", size, (0, 0, 2, 2), None, filter="bilinear_aa")
    arr, n = N.roi_array(rois)
    pairs, used, total = 1, 0, 0
    for i in range(n):
        words = lib.p264hip_roi_aa_segment_words(C.byref(arr[i]), C.byref(r))
        assert words > 0
        if used + words > N.ROI_SCRATCH_BYTES // 4:
            pairs, used = pairs + 1, 0
        used += words
        total += words
    return pairs, total


def tile_widths(lib, rois, size):
    """{tile width: ROIs} as k_roi_aa_* run them"""
    import ctypes as C
    from p264decoder_amd import _native as N
    r = N.resize_desc("rgbp", size, (0, 0, 2, 2), None, filter="bilinear_aa")
    arr, n = N.roi_array(rois)
    hist = {}
    for i in range(n):
        tw = lib.p264hip_roi_aa_tile_width(C.byref(arr[i]), C.byref(r), None, None)
        hist[tw] = hist.get(tw, 0) + 1
    return {str(k): hist[k] for k in sorted(hist)}


def aa_cases(args, hip, streams, slots, scale, bias):
    """the three shapes with filter 2, each beside filter 0 and - whole frames - beside export_resized with filter 2"""
    import numpy as np
    import torch
    from p264decoder_amd import letterbox
    n = args.frames
    src = W * H * 3 // 2
    res = {"metric": "antialiased export of per-picture windows out of %d 1080p frames" % n, "unit": "pictures/s", "frames": n, "reps": args.reps, "warmup": args.warmup, "cases": {}}

    def mem(t):
        return (t.data_ptr(), t.numel() * t.element_size())

    def table(rois, size, dtype, fill, sb, out, extra=None):
        roads = {"aa": lambda: hip.export_rois_aa(rois, size, "rgbp", dtype, fill, sb[0], sb[1], out=mem(out)),
                 "bilinear": lambda: hip.export_rois(rois, size, "rgbp", dtype, fill, sb[0], sb[1], out=mem(out))}
        roads.update(extra or {})
        return alternating(roads, args.warmup, args.reps)

    if "a" in args.only:
        out = torch.empty((n, 3, 224, 224), dtype=torch.float32, device="cuda")
        rois = np.array([(s, k, 0, 0, W, H) for s, k in zip(streams, slots)], np.int32)
        t = table(rois, (224, 224), "f32", (16, 128, 128), (scale, bias), out,
                  {"resized_aa": lambda: hip.export_resized(streams, slots, (224, 224), "rgbp", "f32", (0, 0, W, H), scale, bias, out=mem(out), filter="bilinear_aa")})
        moved = n * (src + 3 * 224 * 224 * 4)
        pairs, words = launch_pairs(hip.lib, rois, (224, 224))
        res["cases"]["a_whole_frames_rgbp_f32_224x224_normalised"] = {
            "p264hip_export_rois_aa": entry(n, t["aa"], moved), "p264hip_export_rois_filter_0": entry(n, t["bilinear"]),
            "p264hip_export_resized_filter_2": entry(n, t["resized_aa"], moved),
            "cost_over_filter_0": round(t["aa"][0] / t["bilinear"][0], 2), "time_over_export_resized_filter_2": round(t["aa"][0] / t["resized_aa"][0], 3),
            "launch_pairs": pairs, "segment_words": words, "tile_widths": tile_widths(hip.lib, rois[:1], (224, 224))}
        res["value"] = res["cases"]["a_whole_frames_rgbp_f32_224x224_normalised"]["p264hip_export_rois_aa"]["frames_per_s"]
        del out
    if "b" in args.only:
        g = np.random.default_rng(2663)                     # (the windows of case b above)
        m = 2 * n
        ww, wh = 2 * g.integers(32, 257, m), 2 * g.integers(32, 257, m)
        left, top = 2 * (g.integers(0, 1 << 30, m) % ((W - ww) // 2 + 1)), 2 * (g.integers(0, 1 << 30, m) % ((H - wh) // 2 + 1))
        rois = np.stack([np.arange(m) // 2, np.arange(m) & 1, left, top, ww, wh], axis=1).astype(np.int32)
        out = torch.empty((m, 3, 224, 224), dtype=torch.float32, device="cuda")
        t = table(rois, (224, 224), "f32", (16, 128, 128), (scale, bias), out)
        read = int((rois[:, 4].astype(np.int64) * rois[:, 5] * 3 // 2).sum())
        pairs, words = launch_pairs(hip.lib, rois, (224, 224))
        res["cases"]["b_drawn_windows_rgbp_f32_224x224_normalised"] = {
            "windows": m, "window_side": "64 .. 512, even, seeded", "p264hip_export_rois_aa_one_call": entry(m, t["aa"], read + m * 3 * 224 * 224 * 4),
            "p264hip_export_rois_filter_0_one_call": entry(m, t["bilinear"]), "cost_over_filter_0": round(t["aa"][0] / t["bilinear"][0], 2),
            "launch_pairs": pairs, "segment_words": words, "tile_widths": tile_widths(hip.lib, rois, (224, 224))}
        del out
    if "c" in args.only:
        rect = letterbox(W, H, 640, 640)
        boxed = torch.empty((n, 3, 640, 640), dtype=torch.float16, device="cuda")
        rois = np.array([(s, k, 0, 0, W, H) + rect for s, k in zip(streams, slots)], np.int32)
        strip = torch.empty((n, 3, 360, 640), dtype=torch.float16, device="cuda")
        t = table(rois, (640, 640), "f16", (16, 128, 128), (1 / 255, 0.0), boxed,
                  {"resized_aa": lambda: hip.export_resized(streams, slots, (640, 360), "rgbp", "f16", (0, 0, W, H), 1 / 255, 0.0, out=mem(strip), filter="bilinear_aa")})
        hip.export_rois_aa(rois, (640, 640), "rgbp", "f16", (16, 128, 128), 1 / 255, 0.0, out=mem(boxed))         # (the last road into `boxed` was filter 0)
        same = bool(torch.equal(boxed[:, :, rect[1]:rect[1] + rect[3], :], strip))
        pairs, words = launch_pairs(hip.lib, rois, (640, 640))
        res["cases"]["c_letterbox_rgbp_f16_640x640"] = {
            "rectangle": list(rect), "p264hip_export_rois_aa": entry(n, t["aa"], n * (src + 3 * 640 * 640 * 2)),
            "p264hip_export_rois_filter_0": entry(n, t["bilinear"]), "cost_over_filter_0": round(t["aa"][0] / t["bilinear"][0], 2),
            "p264hip_export_resized_filter_2_to_640x360_without_the_bars": entry(n, t["resized_aa"]),
            "time_over_export_resized_filter_2_without_the_bars": round(t["aa"][0] / t["resized_aa"][0], 3), "the_rectangle_is_export_resized_filter_2": same,
            "launch_pairs": pairs, "segment_words": words, "tile_widths": tile_widths(hip.lib, rois[:1], (640, 640))}
    return res


def device_cases(args, hip, scale, bias):
    """case b's windows from a list in device memory, beside the host list and beside tensor -> host -> host list"""
    import time
    import statistics
    import numpy as np
    import torch
    from p264decoder_amd import _native as N
    n = args.frames
    g = np.random.default_rng(2663)                         # (the windows of case b)
    m = 2 * n
    ww, wh = 2 * g.integers(32, 257, m), 2 * g.integers(32, 257, m)
    left, top = 2 * (g.integers(0, 1 << 30, m) % ((W - ww) // 2 + 1)), 2 * (g.integers(0, 1 << 30, m) % ((H - wh) // 2 + 1))
    rois = np.stack([np.arange(m) // 2, np.arange(m) & 1, left, top, ww, wh] + [np.zeros(m, np.int64)] * 4, axis=1).astype(np.int32)
    dev = torch.tensor(rois, dtype=torch.int32, device="cuda")
    status = torch.empty(m, dtype=torch.int32, device="cuda")
    out = torch.empty((m, 3, 224, 224), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    mem = (out.data_ptr(), out.numel() * out.element_size())
    lst = (dev.data_ptr(), m)
    size = (224, 224)

    def host(call, sync=True):
        return lambda: call(rois, size, "rgbp", "f32", (16, 128, 128), scale, bias, out=mem, sync=sync)

    def device(filter, reduction, sync=True):
        return lambda: hip.export_rois_device(lst, size, "rgbp", "f32", (16, 128, 128), scale, bias, out=mem, status=status.data_ptr(), filter=filter, max_reduction=reduction,
                                              stream=None, sync=sync)

    def from_tensor(call):
        def road():
            rows = dev.cpu().tolist()
            call([tuple(r) for r in rows], size, "rgbp", "f32", (16, 128, 128), scale, bias, out=mem)
        return road
    roads = {"filter_0_host_list": (host(hip.export_rois), host(hip.export_rois, False), 0, None),
             "filter_0_device_list": (device("bilinear", 0), device("bilinear", 0, False), 0, 0),
             "filter_0_tensor_to_host_then_host_list": (from_tensor(hip.export_rois), None, 0, None),
             "filter_2_host_list": (host(hip.export_rois_aa), host(hip.export_rois_aa, False), 2, None),
             "filter_2_device_list_max_reduction_0": (device("bilinear_aa", 0), device("bilinear_aa", 0, False), 2, 0),
             "filter_2_device_list_max_reduction_3": (device("bilinear_aa", 3), device("bilinear_aa", 3, False), 2, 3),
             "filter_2_tensor_to_host_then_host_list": (from_tensor(hip.export_rois_aa), None, 2, None)}
    t = alternating({k: v[0] for k, v in roads.items()}, args.warmup, args.reps)
    assert status.cpu().eq(0).all()
    # the wall time until the call returns, nothing waited for (a sync, not timed, behind each)
    back = {k: [] for k, v in roads.items() if v[1]}
    for _ in range(args.reps):
        for k in back:
            t0 = time.perf_counter()
            roads[k][1]()
            back[k].append((time.perf_counter() - t0) * 1e3)
            hip.sync()
    read = int((rois[:, 4].astype(np.int64) * rois[:, 5] * 3 // 2).sum())
    res = {"metric": "export of %d drawn windows (64 .. 512 a side) of %d 1080p frames to 224 x 224 planar RGB float32, the ROI list in device memory" % (m, n), "unit": "pictures/s",
           "frames": n, "windows": m, "reps": args.reps, "warmup": args.warmup, "roads": {}}
    for k, (_, _, filter, reduction) in roads.items():
        e = entry(m, t[k], read + m * 3 * 224 * 224 * 4)
        if k in back:
            e["ms_until_the_call_returns"] = {"median": round(statistics.median(back[k]), 3), "min": round(min(back[k]), 3), "max": round(max(back[k]), 3)}
        if reduction is not None:
            plan = N.rois_device_plan(N.resize_desc("rgbp", size, (0, 0, 2, 2), None, filter=filter), reduction, hip.lib)
            e.update(launch_pairs=-(-m // plan["rois_per_pair"]), scratch_bytes_of_a_pair=4 * plan["seg_words"] * min(m, plan["rois_per_pair"]), plan=plan)
        elif filter == 2:
            pairs, words = launch_pairs(hip.lib, rois[:, :6], size)
            e.update(launch_pairs=pairs, scratch_bytes_of_all_segments=4 * words)
        else:
            e.update(launch_pairs=1, scratch_bytes_of_all_segments=4 * 672 * m)
        res["roads"][k] = e
    r = res["roads"]
    res["device_over_host_list_rate"] = {"filter_0": round(r["filter_0_device_list"]["frames_per_s"] / r["filter_0_host_list"]["frames_per_s"], 3),
                                         "filter_2_max_reduction_0": round(r["filter_2_device_list_max_reduction_0"]["frames_per_s"] / r["filter_2_host_list"]["frames_per_s"], 3),
                                         "filter_2_max_reduction_3": round(r["filter_2_device_list_max_reduction_3"]["frames_per_s"] / r["filter_2_host_list"]["frames_per_s"], 3)}
    res["value"] = r["filter_2_device_list_max_reduction_3"]["frames_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048, help="frames of the store = streams of the context (2 slots each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result there")
    ap.add_argument("--only", default="abc", help="the cases to run")
    ap.add_argument("--aa-out", default=None, help="measure the antialiased filter too and write its table there")
    ap.add_argument("--only-aa", action="store_true", help="with --aa-out: skip the filter-0 cases against the roads that existed before")
    ap.add_argument("--device-out", default=None, help="measure the ROI list in device memory too and write its table there")
    ap.add_argument("--only-device", action="store_true", help="with --device-out: skip every other case")
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("roi_bench: no GPU - there is nothing to measure without one")
    from p264decoder_amd import HipReconstructor, letterbox
    n = args.frames
    hip = HipReconstructor(MB_W, MB_H, n_streams=n, slots=2, max_pictures=1)
    streams, slots = list(range(n)), [i & 1 for i in range(n)]
    scale, bias = [1 / (255 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)]
    src = W * H * 3 // 2                       # bytes of a whole picture in the frame store
    res = {"metric": "export of per-picture windows out of %d 1080p frames" % n, "unit": "pictures/s", "frames": n, "reps": args.reps, "warmup": args.warmup, "cases": {}}

    def mem(t):
        return (t.data_ptr(), t.numel() * t.element_size())

    if args.device_out:
        dv = device_cases(args, hip, scale, bias)
        with open(args.device_out, "w") as f:
            f.write(json.dumps(dv) + "\n")
        if args.only_device:
            hip.close()
            print(json.dumps(dv))
            return
    if args.aa_out:
        aa = aa_cases(args, hip, streams, slots, scale, bias)
        with open(args.aa_out, "w") as f:
            f.write(json.dumps(aa) + "\n")
        if args.only_aa:
            hip.close()
            print(json.dumps(aa))
            return
    if "a" in args.only:
        out = torch.empty((n, 3, 224, 224), dtype=torch.float32, device="cuda")
        rois = np.array([(s, k, 0, 0, W, H) for s, k in zip(streams, slots)], np.int32)
        t = alternating({"rois": lambda: hip.export_rois(rois, (224, 224), "rgbp", "f32", scale=scale, bias=bias, out=mem(out)),
                         "resized": lambda: hip.export_resized(streams, slots, (224, 224), "rgbp", "f32", (0, 0, W, H), scale, bias, out=mem(out))}, args.warmup, args.reps)
        moved = n * (src + 3 * 224 * 224 * 4)
        ratio = round(t["resized"][0] / t["rois"][0], 3)
        res["cases"]["a_whole_frames_rgbp_f32_224x224_normalised"] = {
            "p264hip_export_rois": entry(n, t["rois"], moved), "p264hip_export_resized": entry(n, t["resized"], moved),
            "rate_over_export_resized": ratio, "required": 0.9, "met": ratio >= 0.9}
        res["value"] = res["cases"]["a_whole_frames_rgbp_f32_224x224_normalised"]["p264hip_export_rois"]["frames_per_s"]
        del out
    if "b" in args.only:
        g = np.random.default_rng(2663)
        m = 2 * n
        ww, wh = 2 * g.integers(32, 257, m), 2 * g.integers(32, 257, m)
        left, top = 2 * (g.integers(0, 1 << 30, m) % ((W - ww) // 2 + 1)), 2 * (g.integers(0, 1 << 30, m) % ((H - wh) // 2 + 1))
        rois = np.stack([np.arange(m) // 2, np.arange(m) & 1, left, top, ww, wh], axis=1).astype(np.int32)
        assert rois[:, 4].min() >= 64 and rois[:, 4].max() <= 512 and np.all(rois[:, 2] + rois[:, 4] <= W) and np.all(rois[:, 3] + rois[:, 5] <= H)
        out = torch.empty((m, 3, 224, 224), dtype=torch.float32, device="cuda")
        per = 3 * 224 * 224 * 4
        first = [tuple(int(v) for v in r) for r in rois[:PER_CALL]]

        def one_by_one():
            for i, r in enumerate(first):
                hip.export_resized([r[0]], [r[1]], (224, 224), "rgbp", "f32", r[2:], scale, bias, out=(out.data_ptr() + i * per, per), sync=False)
            hip.sync()
        t = alternating({"rois": lambda: hip.export_rois(rois, (224, 224), "rgbp", "f32", scale=scale, bias=bias, out=mem(out)), "one_by_one": one_by_one}, args.warmup, args.reps)
        read = int((rois[:, 4].astype(np.int64) * rois[:, 5] * 3 // 2).sum())
        read_first = int((rois[:PER_CALL, 4].astype(np.int64) * rois[:PER_CALL, 5] * 3 // 2).sum())
        a, b = entry(m, t["rois"], read + m * per), entry(PER_CALL, t["one_by_one"], read_first + PER_CALL * per)
        res["cases"]["b_drawn_windows_rgbp_f32_224x224_normalised"] = {
            "windows": m, "window_side": "64 .. 512, even, seeded", "p264hip_export_rois_one_call": a,
            "p264hip_export_resized_one_call_per_window": dict(b, windows_measured=PER_CALL),
            "rate_over_one_call_per_window": round(a["frames_per_s"] / b["frames_per_s"], 2)}
        del out
    if "c" in args.only:
        rect = letterbox(W, H, 640, 640)
        assert rect == (0, 140, 640, 360)
        boxed = torch.empty((n, 3, 640, 640), dtype=torch.float16, device="cuda")
        strip = torch.empty((n, 3, 360, 640), dtype=torch.float16, device="cuda")
        rois = np.array([(s, k, 0, 0, W, H) + rect for s, k in zip(streams, slots)], np.int32)
        keep = []

        def pad_road():
            hip.export_resized(streams, slots, (640, 360), "rgbp", "f16", (0, 0, W, H), 1 / 255, 0.0, out=mem(strip))
            keep[:] = [F.pad(strip, (0, 0, rect[1], 640 - rect[1] - rect[3]), value=0.0)]       # (fill (16, 128, 128) is RGB 0, 0, 0)
            torch.cuda.synchronize()
        t = alternating({"rois": lambda: hip.export_rois(rois, (640, 640), "rgbp", "f16", (16, 128, 128), 1 / 255, 0.0, out=mem(boxed)), "pad": pad_road}, args.warmup, args.reps)
        same = bool(torch.equal(keep[0], boxed))
        res["cases"]["c_letterbox_rgbp_f16_640x640"] = {
            "rectangle": list(rect), "p264hip_export_rois": entry(n, t["rois"], n * (src + 3 * 640 * 640 * 2)),
            "export_resized_640x360_then_torch_pad": entry(n, t["pad"], n * (src + 2 * 3 * 360 * 640 * 2 + 3 * 640 * 640 * 2)),
            "rate_over_resized_then_pad": round(t["pad"][0] / t["rois"][0], 2), "the_two_roads_agree": same}
    hip.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
