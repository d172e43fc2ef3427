#!/usr/bin/env python3
"""End-to-end rate of the multi-stream pipeline (include/p264pipe.h): Annex-B bytes in host memory -> pictures in HBM,
host CAVLC parse included.  This is NOT bench.py's metric (which times the reconstruction with inputs resident in HBM);
it is the PCIe- and parse-inclusive figure DESIGN.md quotes next to it.

  python -m p264decoder_amd.tools.pipe_bench [--streams 64] [--threads 16] [--pictures 24] [--device 0|-1]
  python -m p264decoder_amd.tools.pipe_bench --output-order [--out profiles/output_order_bench.json]
      the rate with an NV12 sink in decode order beside the rate with the same sink in display order (p264pipe_set_output_order,
      depth 0: the bench stream is all-P, so it is the same pictures in the same order plus the bookkeeping, 17 frame-store slots
      per stream instead of 2, and one export and marker per delivery), alternating, --reps times each
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def output_order(args, streams):
    """decode order and display order side by side, both with an NV12 sink that only counts"""
    from p264decoder_amd import Pipeline
    rates = {"decode_order": [], "output_order": []}
    for rep in range(args.reps + 1):                              # (the first pair is the warm-up)
        for kind in rates:
            pipe = Pipeline(streams, threads=args.threads, device=args.device)
            if kind == "output_order":
                pipe.set_output_order(0)
            got = [0]

            def sink(number, which, dev, per):
                got[0] += len(which)
            pipe.set_sink("nv12", sink)
            st = pipe.run()
            pipe.close()
            assert got[0] == st["pictures"]
            if rep:
                rates[kind].append(round(st["pictures"] / st["seconds"], 1))
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    out = {"metric": "end-to-end 1080p frames/sec with an NV12 sink, decode order beside display order (depth 0)", "unit": "frames/s",
           "streams": args.streams, "threads": args.threads, "pictures_per_stream": args.pictures, "reps": args.reps, "rates": rates, "median": med,
           "output_order_over_decode_order": round(med["output_order"] / med["decode_order"], 4)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 8)
    ap.add_argument("--pictures", type=int, default=24)
    ap.add_argument("--device", type=int, default=0, help="-1: parsers only")
    ap.add_argument("--output-order", action="store_true", help="an NV12 sink in decode order beside the same sink in display order")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="with --output-order: write the result there too")
    args = ap.parse_args()
    import bench
    from p264decoder_amd import Pipeline
    from tests import synth_cases
    distinct = [open(synth_cases.generate(bench.synth_args(args.pictures, 1000 + g)), "rb").read() for g in range(4)]
    if args.output_order:
        import torch  # noqa: F401  (before the library is loaded: one HIP runtime, _native.import_torch)
        return output_order(args, [distinct[i % 4] for i in range(args.streams)])
    pipe = Pipeline([distinct[i % 4] for i in range(args.streams)], threads=args.threads, device=args.device)
    pipe.run(max_pictures=2)                                      # warm-up: contexts, pinned buffers, first launches
    pipe.close()
    pipe = Pipeline([distinct[i % 4] for i in range(args.streams)], threads=args.threads, device=args.device)
    st = pipe.run()
    pipe.close()
    print(json.dumps({"metric": "end-to-end 1080p frames/sec (Annex-B in host memory -> pictures in HBM)",
                      "value": round(st["pictures"] / st["seconds"], 1), "unit": "frames/s",
                      "streams": args.streams, "threads": st["threads"], "pictures": st["pictures"], "device": args.device,
                      "parse_cpu_seconds": round(st["parse_seconds"], 3), "submit_seconds": round(st["submit_seconds"], 3),
                      "wall_seconds": round(st["seconds"], 3), "mbit_per_s": round(st["bytes"] * 8 / st["seconds"] / 1e6, 1)}))


if __name__ == "__main__":
    main()
