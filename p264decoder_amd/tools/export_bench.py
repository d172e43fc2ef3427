#!/usr/bin/env python3
"""Rate of the device export (p264hip_export_frames): a batch of 1080p frames out of the frame stores into device memory,
window 1920 x 1080, as I420 / NV12 / RGB24 / planar RGB - beside the road that existed before it for the same bytes, one
p264hip_frame_planar_device call per frame (uncropped I420).  This is NOT bench.py's metric (the reconstruction); it is the figure
DESIGN.md quotes for the exit.  Every repetition is closed by a sync; the median of --reps is reported.

  python -m p264decoder_amd.tools.export_bench [--frames 2048] [--reps 20] [--warmup 3] [--out profiles/export_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MB_W, MB_H, W, H = 120, 68, 1920, 1080


def timed(fn, sync, warmup, reps):
    for _ in range(warmup):
        fn()
        sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048, help="pictures of a batch = streams of the context (2 slots each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result there")
    args = ap.parse_args()
    import torch
    from p264decoder_amd import HipReconstructor
    n = args.frames
    hip = HipReconstructor(MB_W, MB_H, n_streams=n, slots=2, max_pictures=1)
    streams, slots = list(range(n)), [i & 1 for i in range(n)]
    out = torch.empty(n * W * H * 3, dtype=torch.uint8, device="cuda")           # room for the largest format
    torch.cuda.synchronize()
    res = {"metric": "device export of 1080p frames (window %dx%d, batch of %d)" % (W, H, n), "unit": "frames/s", "frames": n, "reps": args.reps, "formats": {}}
    for fmt in ("i420", "nv12", "rgb24", "rgbp"):
        med, lo, hi = timed(lambda: hip.export_frames(streams, slots, fmt, (0, 0, W, H), out=(out.data_ptr(), out.numel()), sync=False), hip.sync, args.warmup, args.reps)
        moved = n * (W * H * 3 // 2 + (W * H * 3 if fmt.startswith("rgb") else W * H * 3 // 2))
        res["formats"][fmt] = {"ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "frames_per_s": round(n / med * 1e3, 1),
                               "read_plus_written_tb_per_s": round(moved / med / 1e9, 3)}
    # the road of before: one launch per frame, MB-aligned I420 into a buffer of the context's pool each
    per_frame = min(n, 4096)

    def road():
        for i in range(per_frame):
            hip.frame_planar_device(streams[i], slots[i], i)
    med, lo, hi = timed(road, hip.sync, args.warmup, args.reps)
    moved = per_frame * MB_W * MB_H * 384 * 2
    res["per_frame_road_i420"] = {"calls": per_frame, "ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                                  "frames_per_s": round(per_frame / med * 1e3, 1), "read_plus_written_tb_per_s": round(moved / med / 1e9, 3)}
    res["value"] = res["formats"]["i420"]["frames_per_s"]
    res["i420_speedup_over_per_frame_road"] = round(res["per_frame_road_i420"]["ms_per_batch"] / per_frame / (res["formats"]["i420"]["ms_per_batch"] / n), 2)
    hip.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
