#!/usr/bin/env python3
"""Fullcolor (4:4:4) against 4:2:0 on a video pipeline, same process,
same frames, alternating the two modes: H.264 (Hi444 separate colour
planes, --output-mode 1, the default) or HEVC (Main 4:4:4,
--output-mode 2).

    python tools/bench_fullcolor.py --kind gpu --width 1920 --height 1080 \\
        --depth 1 --steps 600 --repeats 3 [--output-mode 2]

Both modes run through _native.BenchPipeline on worst-case input (every
pixel of every frame random). One repeat is a timed window of --steps
frames per mode, fullcolor then 4:2:0; the windows alternate so drift on
a shared host lands on both. A window is timed with a host clock around
encode calls that end in the frame's bytes being on the host (depth 1),
closed by a flush and a device synchronise; p50 is the median
submit-to-emitted time of a frame. Prints one JSON line per window and a
summary line with the median fps of each mode, the min..max spread over
the repeats, and the fullcolor / 4:2:0 ratio.

--kind gpu fails when there is no HIP device: it never falls back."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["gpu", "cpu"], required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=1, choices=[1, 2],
                    help="pipeline depth (2 keeps one frame in flight)")
    ap.add_argument("--steps", type=int, default=600,
                    help="timed frames per window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--qp", type=int, default=28)
    ap.add_argument("--output-mode", type=int, default=1, choices=[1, 2],
                    help="1 = H.264 (default), 2 = HEVC")
    args = ap.parse_args()

    gpu = args.kind == "gpu"
    if gpu:
        # torch brings its own HIP runtime up first, as in bench.py; it
        # serves only as the device synchronise around the timed windows
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_fullcolor: --kind gpu but no HIP device is "
                     "present")
        torch.cuda.set_device(0)
        torch.cuda.synchronize()

    import hipflux
    from hipflux import _native

    if gpu and hipflux.hip_device_count() == 0:
        sys.exit("bench_fullcolor: --kind gpu but no HIP device is present")

    def device_sync():
        if gpu:
            torch.cuda.synchronize()

    rng = np.random.default_rng(1234)
    n_src = min(24, max(4, args.warmup))
    frames = [rng.integers(0, 256, (args.height, args.width, 4),
                           dtype=np.uint8) for _ in range(n_src)]

    pipes = {}
    for mode, fc in (("fullcolor", True), ("420", False)):
        p = _native.BenchPipeline(args.kind, args.width, args.height,
                                  qp=args.qp, stripe_height=64,
                                  output_mode=args.output_mode,
                                  gpu_id=0 if gpu else -1,
                                  pipeline_depth=args.depth, fullcolor=fc)
        codec = "h264" if args.output_mode == 1 else "hevc"
        want = f"hip-{codec}" if gpu else f"cpu-{codec}"
        if p.pipeline != want:
            sys.exit(f"bench_fullcolor: {mode} runs on {p.pipeline}, "
                     f"not {want}")
        # warmup (untimed): the IDR, allocations, every source frame once
        p.encode(frames[0], True)
        for i in range(max(1, args.warmup - 1)):
            p.encode(frames[(i + 1) % n_src], False)
        p.flush()
        pipes[mode] = [p, 1 + max(1, args.warmup - 1)]
    device_sync()

    def window(mode):
        p, next_fid = pipes[mode]
        starts, lat_ms, nbytes = {}, [], 0
        device_sync()
        t0 = time.perf_counter()
        for i in range(args.steps):
            starts[next_fid] = time.perf_counter()
            next_fid += 1
            b, _ = p.encode(frames[i % n_src], False)
            nbytes += b
            done = p.last_frame_id
            if done in starts:
                lat_ms.append((time.perf_counter() - starts.pop(done)) * 1e3)
        b, _ = p.flush()
        nbytes += b
        done = p.last_frame_id
        if done in starts:
            lat_ms.append((time.perf_counter() - starts.pop(done)) * 1e3)
        device_sync()
        t1 = time.perf_counter()
        pipes[mode][1] = next_fid
        return {"mode": mode, "fps": round(args.steps / (t1 - t0), 2),
                "p50_ms": round(statistics.median(lat_ms), 3),
                "window_s": round(t1 - t0, 3),
                "mbit_per_frame": round(nbytes * 8e-6 / args.steps, 3)}

    results = {"fullcolor": [], "420": []}
    for rep in range(args.repeats):
        for mode in ("fullcolor", "420"):
            r = window(mode)
            results[mode].append(r)
            print(json.dumps(dict(r, rep=rep, kind=args.kind,
                                  depth=args.depth,
                                  output_mode=args.output_mode)), flush=True)

    def med(mode, key):
        return statistics.median(r[key] for r in results[mode])

    summary = {"kind": args.kind, "output_mode": args.output_mode,
               "width": args.width, "height": args.height,
               "depth": args.depth, "steps": args.steps,
               "repeats": args.repeats, "qp": args.qp}
    for mode in ("fullcolor", "420"):
        fps = [r["fps"] for r in results[mode]]
        summary[mode] = {"fps": med(mode, "fps"), "fps_min": min(fps),
                         "fps_max": max(fps), "p50_ms": med(mode, "p50_ms")}
    summary["fullcolor_over_420"] = round(
        summary["fullcolor"]["fps"] / summary["420"]["fps"], 3)
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
