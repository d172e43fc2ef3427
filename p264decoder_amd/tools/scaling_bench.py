#!/usr/bin/env python3
"""Rate of the reconstruction of P pictures with and without scaling matrices: bench.py's 1080p all-P configuration (its writer
options: 120 x 68 macroblocks, CAVLC, one IDR picture then P pictures) written as High profile, once flat and once with --cqm jvt (the
default lists of tables 7-3 / 7-4 in the SPS: every picture has scaling_lists, the batch launches k_mc_sort_scaled, k_scaled_inter and
k_intra_sparse_scaled), at 256 and at 2048 pictures per launch in one context, inputs resident, --runs runs each.  Only the P
launches are timed; the stage times are the context's HIP events (inter = sort + motion compensation + k_scaled_inter).  This is NOT
bench.py's metric and has no pass mark: it is the pair DESIGN.md quotes for the extra pass.  Nothing checks the pictures here (the
tests do).  --t8x8 PCT gives that share of the inter macroblocks the 8x8 transform: the flat batch then launches k_t8x8, and
k_scaled_inter walks 8x8 blocks too; the default 0 is the stream of the committed figures.  A third variant, cr_offset: the flat stream
with --cqo2 different from --cqo (every picture has a cr_qp_offset_delta: the scaled road with the all-16 table, and the Cr instances
of the loop filter, k_deblock_bs_cr and k_deblock_cr) - what such a picture costs, against the flat and the scaled variant of the same run.

  python -m p264decoder_amd.tools.scaling_bench [--streams 256 2048] [--pictures 5] [--runs 3] [--t8x8 0] [--out profiles/scaling_bench.json]
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

MB_W, MB_H = 120, 68
OPTIONS = "--mbw %d --mbh %d --gop 0 --seed 33 --coded 12 --maxlevel 12 --crop-bottom 4 --t8x8 %%d" % (MB_W, MB_H)     # (--t8x8 PCT: main)
CASES = (("flat", ""), ("cqm_jvt", "--cqm jvt --cqm-where sps"), ("cr_offset", "--cqo 2 --cqo2 -3"))


def one_run(hip, S, T):
    """the IDR launch untimed, then the T - 1 P launches: (frames/s, {stage: ms per launch})"""
    streams = list(range(S))
    hip.reconstruct([s * T for s in streams], streams)
    hip.sync()
    hip.timing_reset()
    t0 = time.perf_counter()
    for t in range(1, T):
        hip.reconstruct([s * T + t for s in streams], streams)
    hip.sync()
    dt = time.perf_counter() - t0
    stages = {k: round(ms / max(n, 1), 4) for k, (ms, n) in hip.timing_read().items()}
    return S * (T - 1) / dt, stages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[256, 2048], help="pictures of a batch = streams of the context")
    ap.add_argument("--pictures", type=int, default=5, help="pictures per stream: one IDR picture and the P launches of a run")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--t8x8", type=int, default=0, metavar="PCT", help="per cent of the inter macroblocks coded with the 8x8 transform")
    ap.add_argument("--out", default=None, help="also write the result there")
    args = ap.parse_args()
    from p264decoder_amd import HipReconstructor, Parser
    from p264decoder_amd import build as _build
    tool = os.path.join(os.path.dirname(_build.__file__), "tools", "synth264")
    if not os.path.exists(tool):
        _build.build_tools()
    T = args.pictures
    options = OPTIONS % args.t8x8
    res = {"metric": "reconstruction of 1080p P pictures (bench.py's all-P stream as High profile), inputs resident, P launches only", "unit": "frames/s",
           "pictures_per_stream": T, "runs": args.runs, "stream_options": options, "batches": {}}
    with tempfile.TemporaryDirectory() as td:
        parsed = {}
        for name, extra in CASES:
            path = os.path.join(td, name + ".264")
            subprocess.run([tool, path] + options.split() + ["--frames", str(T)] + extra.split(), check=True)
            parsed[name] = Parser(quiet=True, intra8x8=True, scaling=True, cr_offset=True).parse_stream(open(path, "rb").read())
            assert len(parsed[name]) == T and all(bool(p.desc.scaling_lists) == ("--cqm" in extra) for p in parsed[name])
            assert all(bool(p.desc.cr_qp_offset_delta) == ("--cqo2" in extra) for p in parsed[name])
        for S in args.streams:
            out = res["batches"][str(S)] = {}
            for name, _ in CASES:
                pics = parsed[name]
                hip = HipReconstructor(MB_W, MB_H, n_streams=S, slots=2, max_pictures=S * T)
                hip.timing_enable(True)
                hip.upload(0, pics)
                for s in range(1, S):
                    for t in range(T):
                        hip.clone_picture(s * T + t, t)
                hip.sync()
                one_run(hip, S, T)                              # untimed: allocations, first launches
                runs = [one_run(hip, S, T) for _ in range(args.runs)]
                fps = [r[0] for r in runs]
                out[name] = {"frames_per_s": [round(f, 1) for f in fps], "median": round(statistics.median(fps), 1),
                             "stage_ms_per_launch": runs[[round(f, 1) for f in fps].index(round(statistics.median(fps), 1))][1],
                             "scaled_pictures_per_launch": hip.last_scaled_pictures(), "cr_pictures_per_launch": hip.last_cr_pictures(), "coded_blocks_per_picture": int(pics[-1].desc.n_coef_blocks)}
                hip.close()
            out["cqm_relative_to_flat"] = round(out["cqm_jvt"]["median"] / out["flat"]["median"], 3)
            out["cr_offset_relative_to_flat"] = round(out["cr_offset"]["median"] / out["flat"]["median"], 3)
            out["cr_offset_relative_to_cqm"] = round(out["cr_offset"]["median"] / out["cqm_jvt"]["median"], 3)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
