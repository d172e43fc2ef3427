#!/usr/bin/env python3
"""Rate of the resized device export (p264hip_export_resized): a batch of 1080p frames out of the frame stores, window 1920 x 1080,
resized on the device - to 224 x 224 planar RGB as normalised float32, to 224 x 224 planar RGB bytes, to 640 x 360 NV12 - beside the
road that existed before it for the two RGB cases: p264hip_export_frames (planar RGB bytes of the full window) followed by
torch.nn.functional.interpolate(mode="bilinear", align_corners=False) and the normalisation in torch.  The two roads of a case
alternate repetition by repetition in one run.  There was no YUV resize before: the NV12 case stands alone, with the bytes it reads
and writes per second.  This is NOT bench.py's metric (the reconstruction); it is the figure DESIGN.md quotes for K6.  Every repetition
is closed by a sync; the median of --reps is reported with min and max.  Bytes are counted from the shapes.

--aa-out measures the ANTIALIASED filter (filter="bilinear_aa", kernel_resize_aa.h) as well, the same three shapes, each beside two
roads: the same call with filter 0 from this build (what the antialiasing costs) and p264hip_export_frames followed by
torch.nn.functional.interpolate(mode="bilinear", antialias=True) on the device (the road it replaces; the NV12 case exports I420 and
resizes the three planes).  That table goes to the file named, with the bytes per frame and the tile the host chose; --only-aa skips
the cases above.

  python -m p264decoder_amd.tools.resize_bench [--frames 2048] [--reps 20] [--warmup 3] [--out profiles/resize_bench.json]
                                               [--aa-out profiles/resize_aa_bench.json] [--only-aa]
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


def aa_tile(lib, src_w, dst_w):
    """the tile width p264hip_export_resized chooses for the antialiased filter (p264hip.hip: export_resized_aa), luma and chroma spans"""
    import ctypes as C

    def span(S, D, tw, sh):
        first, count, w = (C.c_int32 * D)(), (C.c_int32 * D)(), (C.c_uint16 * (D * 64))()
        assert lib.p264hip_resize_aa_taps(S, D, first, count, w) == 0
        return max(((first[min(x + tw, D) - 1] + count[min(x + tw, D) - 1] - 1) >> sh) - (first[x] >> sh) + 1 for x in range(0, D, tw))
    for tw in (64, 32, 16, 8):
        ns_l, ns_c = span(src_w, dst_w, tw, 4), span(src_w // 2, dst_w // 2, tw // 2, 3)
        if ns_l * 16 * 16 <= 20480 and ns_c * 16 * 8 <= 20480:
            break
    return {"tile_w": tw, "tile_h": 16, "luma_strips_of_a_tile": ns_l, "chroma_strips_of_a_tile": ns_c, "lds_bytes_of_a_workgroup": max(2 * 16 * 16 * ns_l, 2 * 8 * 16 * ns_c)}


def plain_cases(args, n, src, ours, torch_road, small_f, small_u, nv12, scale, bias):
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
    return res


def aa_cases(args, n, src, hip, torch, F, ours, full, small_f, small_u, nv12, scale, bias, t_scale, t_bias, streams, slots, window):
    """the antialiased filter beside filter 0 and beside export + torch's antialiased interpolate"""
    try:
        F.interpolate(torch.zeros(1, 1, 8, 8, device="cuda"), size=(2, 2), mode="bilinear", align_corners=False, antialias=True)
        torch.cuda.synchronize()
        torch_aa = None
    except Exception as e:                      # (a device build without the antialiased kernels: the two other columns stand)
        torch_aa = "torch.nn.functional.interpolate(antialias=True) is not available on this device build: %s" % e

    def resize(x, size):
        return (F.interpolate(x.float(), size=size, mode="bilinear", align_corners=False, antialias=True) + 0.5).clamp_(0, 255)

    def torch_rgb(normalise):
        hip.export_frames(streams, slots, "rgbp", window, out=(full.data_ptr(), full.numel()), sync=True)
        for i in range(0, n, TORCH_CHUNK):
            x = F.interpolate(full[i:i + TORCH_CHUNK].float(), size=(224, 224), mode="bilinear", align_corners=False, antialias=True)
            if normalise:
                small_f[i:i + TORCH_CHUNK] = x * t_scale + t_bias
            else:
                small_u[i:i + TORCH_CHUNK] = (x + 0.5).clamp_(0, 255).to(torch.uint8)
        torch.cuda.synchronize()

    flat = full.view(-1)[:n * src].view(n, src)

    def torch_nv12():
        hip.export_frames(streams, slots, "i420", window, out=(flat.data_ptr(), flat.numel()), sync=True)
        for i in range(0, n, TORCH_CHUNK):
            p = flat[i:i + TORCH_CHUNK]
            k = p.shape[0]
            nv12[i:i + k, :360] = resize(p[:, :W * H].view(k, 1, H, W), (360, 640)).to(torch.uint8)[:, 0]
            c = resize(p[:, W * H:].view(k, 2, H // 2, W // 2), (180, 320)).to(torch.uint8)
            nv12[i:i + k, 360:, 0::2] = c[:, 0]
            nv12[i:i + k, 360:, 1::2] = c[:, 1]
        torch.cuda.synchronize()

    res = {"metric": "antialiased resized device export of 1080p frames (window %dx%d, %d pictures per launch)" % (W, H, n), "unit": "frames/s", "frames": n,
           "reps": args.reps, "warmup": args.warmup, "cases": {}}
    if torch_aa:
        res["torch_note"] = torch_aa
    for name, out, fmt, dtype, size, sb, road, written in (
            ("rgbp_f32_224x224_normalised", small_f, "rgbp", "f32", (224, 224), (scale, bias), lambda: torch_rgb(True), 3 * 224 * 224 * 4),
            ("rgbp_u8_224x224", small_u, "rgbp", "u8", (224, 224), (None, None), lambda: torch_rgb(False), 3 * 224 * 224),
            ("nv12_640x360", nv12, "nv12", "u8", (640, 360), (None, None), torch_nv12, 640 * 360 * 3 // 2)):
        roads = {"aa": lambda: ours(out, fmt, dtype, size, sb, "bilinear_aa"), "bilinear": lambda: ours(out, fmt, dtype, size, sb)}
        if not torch_aa:
            roads["torch"] = road
        t = alternating(roads, args.warmup, args.reps)
        case = {"bytes_read_per_frame": src, "bytes_written_per_frame": written, "tile": aa_tile(hip.lib, W, size[0]),
                "filter_bilinear_aa": entry(n, t["aa"], n * (src + written)), "filter_bilinear": entry(n, t["bilinear"]),
                "cost_over_filter_bilinear": round(t["aa"][0] / t["bilinear"][0], 2)}
        if not torch_aa:
            case["export_frames_then_torch_interpolate_antialias"] = entry(n, t["torch"])
            case["speedup_over_export_then_torch"] = round(t["torch"][0] / t["aa"][0], 2)
        res["cases"][name] = case
    res["value"] = res["cases"]["rgbp_f32_224x224_normalised"]["filter_bilinear_aa"]["frames_per_s"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048, help="pictures of a launch = streams of the context (2 slots each)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result there")
    ap.add_argument("--aa-out", default=None, help="measure the antialiased filter too and write its table there")
    ap.add_argument("--only-aa", action="store_true", help="with --aa-out: skip the filter-0 cases against the plain torch road")
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

    def ours(out, fmt, dtype, size, sb, filter="bilinear"):
        hip.export_resized(streams, slots, size, fmt, dtype, window, sb[0], sb[1], out=(out.data_ptr(), out.numel() * out.element_size()), sync=True, filter=filter)

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
    res = None
    if not (args.aa_out and args.only_aa):
        res = plain_cases(args, n, src, ours, torch_road, small_f, small_u, nv12, scale, bias)
    if args.aa_out:
        aa = aa_cases(args, n, src, hip, torch, F, ours, full, small_f, small_u, nv12, scale, bias, t_scale, t_bias, streams, slots, window)
        with open(args.aa_out, "w") as f:
            f.write(json.dumps(aa) + "\n")
        if res is None:
            res = aa
    hip.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
