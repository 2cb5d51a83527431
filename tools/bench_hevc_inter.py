#!/usr/bin/env python3
"""HEVC with P stripes (hevc_inter) against all-intra HEVC, same process,
same frames, alternating the two modes.

    python tools/bench_hevc_inter.py --kind gpu --width 1920 --height 1080 \\
        --content typing --depth 1 --steps 300 --repeats 3

Contents:
  typing  a static desktop-like frame (flat panels, text-like 1-pixel
          detail) in which one 16x16 block changes per frame; every stripe
          is forced to encode, so the figure is the cost of the unchanged
          CTUs. The claim to confirm: P bytes/frame far below intra.
  noise   worst case, every pixel of every frame random: every P CTU ends
          up intra, so this is the added cost of the reference read, the
          fifth SAD and the P syntax.

Both modes run through _native.BenchPipeline. One repeat is a timed window
of --steps frames per mode, inter then intra; the windows alternate so
drift on a shared host lands on both. A window is timed with a host clock
around encode calls, closed by a flush and a device synchronise. Prints one
JSON line per window and a summary with each mode's median fps, the
min..max spread over the repeats, bytes/frame, and the inter/intra ratios.

--kind gpu fails when there is no HIP device: it never falls back."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def desktop_frame(w, h, rng):
    f = np.zeros((h, w, 4), np.uint8)
    f[:, :, :3] = (236, 236, 240)                       # window background
    f[:h // 16, :, :3] = (60, 60, 70)                   # title bar
    f[:, :w // 6, :3] = (200, 205, 215)                 # side panel
    # text-like rows: 1-pixel dark detail on every third 16-row line
    for y in range(h // 8, h - 16, 48):
        line = rng.integers(0, 2, (10, w - w // 4), dtype=np.uint8)
        f[y:y + 10, w // 5:w // 5 + line.shape[1], :3] = np.where(
            line[:, :, None] == 1, 30, 236)
    f[:, :, 3] = 255
    return f


def typing_frames(w, h, n, rng):
    """n frames: the desktop with one more 16x16 block of 'glyphs' each."""
    base = desktop_frame(w, h, rng)
    frames = []
    cols = (w - w // 4) // 16
    for i in range(n):
        f = base if i == 0 else frames[-1].copy()
        if i:
            x = w // 5 + (i % cols) * 16
            y = (h // 2) & ~15
            f[y:y + 16, x:x + 16, :3] = np.where(
                rng.integers(0, 2, (16, 16, 1), dtype=np.uint8) == 1, 30, 236)
        frames.append(f)
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["gpu", "cpu"], required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--content", choices=["typing", "noise"],
                    default="typing")
    ap.add_argument("--depth", type=int, default=1, choices=[1, 2])
    ap.add_argument("--steps", type=int, default=300,
                    help="timed frames per window")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--qp", type=int, default=28)
    args = ap.parse_args()

    gpu = args.kind == "gpu"
    if gpu:
        # torch brings its own HIP runtime up first, as in bench.py; it
        # serves only as the device synchronise around the timed windows
        import torch
        if not torch.cuda.is_available():
            sys.exit("bench_hevc_inter: --kind gpu but no HIP device is "
                     "present")
        torch.cuda.set_device(0)
        torch.cuda.synchronize()

    import hipflux
    from hipflux import _native

    if gpu and hipflux.hip_device_count() == 0:
        sys.exit("bench_hevc_inter: --kind gpu but no HIP device is present")

    def device_sync():
        if gpu:
            torch.cuda.synchronize()

    rng = np.random.default_rng(1234)
    n_src = 24
    if args.content == "noise":
        frames = [rng.integers(0, 256, (args.height, args.width, 4),
                               dtype=np.uint8) for _ in range(n_src)]
    else:
        frames = typing_frames(args.width, args.height, n_src, rng)

    pipes = {}
    for mode, inter in (("inter", True), ("intra", False)):
        p = _native.BenchPipeline(args.kind, args.width, args.height,
                                  qp=args.qp, stripe_height=64,
                                  output_mode=2, gpu_id=0 if gpu else -1,
                                  pipeline_depth=args.depth,
                                  hevc_inter=inter)
        want = "hip-hevc" if gpu else "cpu-hevc"
        if p.pipeline != want:
            sys.exit(f"bench_hevc_inter: {mode} runs on {p.pipeline}, "
                     f"not {want}")
        p.encode(frames[0], True)          # the IDR, untimed
        for i in range(max(1, args.warmup - 1)):
            p.encode(frames[(i + 1) % n_src], False)
        p.flush()
        pipes[mode] = p
    device_sync()

    def window(mode):
        p = pipes[mode]
        nbytes = 0
        device_sync()
        t0 = time.perf_counter()
        for i in range(args.steps):
            b, _ = p.encode(frames[i % n_src], False)
            nbytes += b
        b, _ = p.flush()
        nbytes += b
        device_sync()
        t1 = time.perf_counter()
        return {"mode": mode, "fps": round(args.steps / (t1 - t0), 2),
                "window_s": round(t1 - t0, 3),
                "bytes_per_frame": round(nbytes / args.steps, 1)}

    results = {"inter": [], "intra": []}
    for rep in range(args.repeats):
        for mode in ("inter", "intra"):
            r = window(mode)
            results[mode].append(r)
            print(json.dumps(dict(r, rep=rep, kind=args.kind,
                                  content=args.content, depth=args.depth)),
                  flush=True)

    summary = {"kind": args.kind, "content": args.content,
               "width": args.width, "height": args.height,
               "depth": args.depth, "steps": args.steps,
               "repeats": args.repeats, "qp": args.qp}
    for mode in ("inter", "intra"):
        fps = [r["fps"] for r in results[mode]]
        summary[mode] = {
            "fps": statistics.median(fps), "fps_min": min(fps),
            "fps_max": max(fps),
            "bytes_per_frame": statistics.median(
                r["bytes_per_frame"] for r in results[mode])}
    summary["inter_over_intra_fps"] = round(
        summary["inter"]["fps"] / summary["intra"]["fps"], 3)
    summary["inter_over_intra_bytes"] = round(
        summary["inter"]["bytes_per_frame"] /
        summary["intra"]["bytes_per_frame"], 4)
    print(json.dumps({"summary": summary}), flush=True)


if __name__ == "__main__":
    main()
