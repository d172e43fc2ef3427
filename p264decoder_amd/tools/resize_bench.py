#!/usr/bin/env python3
"""Rate of the resized device export (p264hip_export_resized): a batch of 1080p frames out of the frame stores, window 1920 x 1080,
resized on the device - to 224 x 224 planar RGB as normalised float32, to 224 x 224 planar RGB bytes, to 640 x 360 NV12 - beside the
road that existed before it for the two RGB cases: p264hip_export_frames (planar RGB bytes of the full window) followed by
torch.nn.functional.interpolate(mode="bilinear", align_corners=False) and the normalisation in torch.  The two roads of a case
alternate repetition by repetition in one run.  There was no YUV resize before: the NV12 case stands alone, with the bytes it reads
and writes per second.  This is NOT bench.py's metric (the reconstruction); it is the figure DESIGN.md quotes for K6.  Every repetition
is closed by a sync; the median of --reps is reported with min and max.  Bytes are counted from the shapes.

  python -m p264decoder_amd.tools.resize_bench [--frames 2048] [--reps 20] [--warmup 3] [--out profiles/resize_bench.json]
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TORCH_CHUNK = 256           # pictures the torch road converts to float at a time (2048 full-size float32 pictures are 51 GB)


def alternating(roads, warmup, reps):
    """roads: {name: callable that returns after its sync}; one repetition of each in turn -> {name: (median, min, max) in ms}"""
    for _ in range(warmup):
        for fn in roads.values():
            fn()
    ms = {k: [] for k in roads}
    for _ in range(reps):
        for k, fn in roads.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def entry(n, t, moved=None):
    med, lo, hi = t
    e = {"ms_per_batch": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "frames_per_s": round(n / med * 1e3, 1)}
    if moved is not None:
        e["bytes_read_plus_written"] = moved
        e["read_plus_written_tb_per_s"] = round(moved / med / 1e9, 3)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048, help="pictures of a launch = streams of the context (2 slots each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result there")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: no GPU - there is nothing to measure without one")
    from p264decoder_amd import HipReconstructor
    n = args.frames
    hip = HipReconstructor(MB_W, MB_H, n_streams=n, slots=2, max_pictures=1)
    streams, slots = list(range(n)), [i & 1 for i in range(n)]
    scale, bias = [1 / (255 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)]
    full = torch.empty((n, 3, H, W), dtype=torch.uint8, device="cuda")                  # the torch road's full-size export
    small_f = torch.empty((n, 3, 224, 224), dtype=torch.float32, device="cuda")
    small_u = torch.empty((n, 3, 224, 224), dtype=torch.uint8, device="cuda")
    nv12 = torch.empty((n, 360 * 3 // 2, 640), dtype=torch.uint8, device="cuda")
    t_scale = torch.tensor(scale, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    t_bias = torch.tensor(bias, dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
    torch.cuda.synchronize()
    window = (0, 0, W, H)

    def ours(out, fmt, dtype, size, sb):
        hip.export_resized(streams, slots, size, fmt, dtype, window, sb[0], sb[1], out=(out.data_ptr(), out.numel() * out.element_size()), sync=True)

    def torch_road(normalise):
        hip.export_frames(streams, slots, "rgbp", window, out=(full.data_ptr(), full.numel()), sync=True)
        for i in range(0, n, TORCH_CHUNK):
            x = F.interpolate(full[i:i + TORCH_CHUNK].float(), size=(224, 224), mode="bilinear", align_corners=False)
            if normalise:
                small_f[i:i + TORCH_CHUNK] = x * t_scale + t_bias
            else:
                small_u[i:i + TORCH_CHUNK] = (x + 0.5).clamp_(0, 255).to(torch.uint8)
        torch.cuda.synchronize()

    src = W * H * 3 // 2                       # bytes of a picture's window in the frame store
    res = {"metric": "resized device export of 1080p frames (window %dx%d, %d pictures per launch)" % (W, H, n), "unit": "frames/s", "frames": n,
           "reps": args.reps, "warmup": args.warmup, "cases": {}}
    t = alternating({"resized": lambda: ours(small_f, "rgbp", "f32", (224, 224), (scale, bias)), "export_then_torch": lambda: torch_road(True)}, args.warmup, args.reps)
    res["cases"]["rgbp_f32_224x224_normalised"] = {
        "p264hip_export_resized": entry(n, t["resized"], n * (src + 3 * 224 * 224 * 4)),
        "export_frames_rgbp_then_torch_interpolate_and_normalise": entry(n, t["export_then_torch"]),
        "speedup": round(t["export_then_torch"][0] / t["resized"][0], 2)}
    t = alternating({"resized": lambda: ours(small_u, "rgbp", "u8", (224, 224), (None, None)), "export_then_torch": lambda: torch_road(False)}, args.warmup, args.reps)
    res["cases"]["rgbp_u8_224x224"] = {
        "p264hip_export_resized": entry(n, t["resized"], n * (src + 3 * 224 * 224)),
        "export_frames_rgbp_then_torch_interpolate_and_round": entry(n, t["export_then_torch"]),
        "speedup": round(t["export_then_torch"][0] / t["resized"][0], 2)}
    t = alternating({"resized": lambda: ours(nv12, "nv12", "u8", (640, 360), (None, None))}, args.warmup, args.reps)
    # (what the kernel can read at most: every source byte once; a reduction by three reads one row in three)
    res["cases"]["nv12_640x360"] = {"p264hip_export_resized": entry(n, t["resized"], n * (src + 640 * 360 * 3 // 2)),
                                    "note": "no YUV resize existed before: reported alone; bytes read counted as the whole window once"}
    res["value"] = res["cases"]["rgbp_f32_224x224_normalised"]["p264hip_export_resized"]["frames_per_s"]
    hip.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
