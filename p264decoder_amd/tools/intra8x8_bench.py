#!/usr/bin/env python3
"""Rate of the reconstruction on intra-only 720p pictures with and without Intra 8x8 macroblocks: synth264 streams with config 2's
options (1280 x 720, CAVLC, I slices only) as High profile, once with --i8x8 0 (no record carries P264_MB_I8X8: the batch launches
k_intra, as config 2 does) and once with --i8x8 50 (half of the I_NxN macroblocks are Intra 8x8: the batch launches k_intra_i8), a
batch of 256 pictures per launch in one context, inputs resident, --runs runs each.  This is NOT bench.py's metric and has no pass
mark: it is the figure DESIGN.md quotes for the Intra 8x8 road beside config 2's.  Nothing checks the pictures here (the tests do).

  python -m p264decoder_amd.tools.intra8x8_bench [--streams 256] [--pictures 6] [--runs 3] [--out profiles/i8x8_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MB_W, MB_H = 80, 45
OPTIONS = "--mbw %d --mbh %d --intra-only --seed 2 --coded 25 --maxlevel 32 --t8x8 0" % (MB_W, MB_H)


def one_run(hip, S, T):
    streams = list(range(S))
    t0 = time.perf_counter()
    for t in range(T):
        hip.reconstruct([s * T + t for s in streams], streams)
    hip.sync()
    return S * T / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256, help="pictures of a batch = streams of the context")
    ap.add_argument("--pictures", type=int, default=6, help="pictures per stream = launches of a run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result there")
    args = ap.parse_args()
    from p264decoder_amd import HipReconstructor, Parser, _native as N
    from p264decoder_amd import build as _build
    tool = os.path.join(os.path.dirname(_build.__file__), "tools", "synth264")
    if not os.path.exists(tool):
        _build.build_tools()
    S, T = args.streams, args.pictures
    res = {"metric": "reconstruction of intra-only 720p CAVLC pictures, batch of %d, inputs resident" % S, "unit": "frames/s", "streams": S,
           "pictures_per_stream": T, "runs": args.runs, "stream_options": OPTIONS, "cases": {}}
    with tempfile.TemporaryDirectory() as td:
        for pct in (0, 50):
            path = os.path.join(td, "i8_%d.264" % pct)
            subprocess.run([tool, path] + OPTIONS.split() + ["--frames", str(T), "--i8x8", str(pct)], check=True)
            pics = Parser(quiet=True, intra8x8=True).parse_stream(open(path, "rb").read())
            assert len(pics) == T
            rec = [p.mb_records() for p in pics]
            share = sum(int(((r["intra_modes"] & N.MB_I8X8) != 0).sum()) for r in rec) / float(sum(len(r) for r in rec))
            hip = HipReconstructor(MB_W, MB_H, n_streams=S, slots=2, max_pictures=S * T)
            hip.upload(0, pics)
            for s in range(1, S):
                for t in range(T):
                    hip.clone_picture(s * T + t, t)
            hip.sync()
            one_run(hip, S, T)                              # untimed: allocations, first launches
            fps = [one_run(hip, S, T) for _ in range(args.runs)]
            res["cases"]["i8x8_%d" % pct] = {"frames_per_s": [round(f, 1) for f in fps], "median": round(statistics.median(fps), 1),
                                             "intra_8x8_share_of_macroblocks": round(share, 3), "intra_i8_launch": hip.last_intra_i8(),
                                             "intra_waves": hip.last_launch()["intra_waves"]}
            hip.close()
    res["value"] = res["cases"]["i8x8_50"]["median"]
    res["relative_to_i8x8_0"] = round(res["cases"]["i8x8_50"]["median"] / res["cases"]["i8x8_0"]["median"], 3)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
