#!/usr/bin/env python3
"""Capture front end on the GPU (_native.GpuFrontEnd: upload, overlay,
downscale, block diff) against the host code it replaces
(_native._frontend_cpu: cpu/overlay.h, cpu/scale.h,
DamageTracker::update), same process, same frames, alternating windows.

    python tools/bench_frontend.py --steps 30 --repeats 3 [--markdown]

For 1920x1080 and 3840x2160, {no scaling, 0.5x bilinear, box /2} x
{static frame, full-noise frames}, cursor on, threshold 15. One repeat is
a timed window of --steps process() calls per path, host then GPU; the
windows alternate so drift on a shared host lands on both. A process()
call ends with its result on the host (the GPU path synchronises its
stream), so a host clock around the window is the time the capture thread
would spend. Reported: median ms/frame over the repeats and the min..max
spread, per path.

The GPU path uploads the NATIVE frame (with scaling on, 4x the bytes of
the scaled upload the host path leaves to the pipeline at 0.5x), so its
figure includes an upload the host figure does not; `h2d` in the stage
breakdown is that upload. To compare like with like the table also gives
`host+up`: the host path plus a pinned upload of its scaled frame,
measured in the same run.

Stage times come from HIP events inside GpuFrontEnd (median over --steps
frames). Each kernel's GB/s (bytes read + written / time) stands next to
a device-to-device hipMemcpyAsync moving the same number of bytes in the
same run: the yardstick for a streaming kernel.

Fails when there is no HIP device: it never falls back."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(1920, 1080), (3840, 2160)]
MODES = [("none", {}), ("bilinear0.5", {"scale": 0.5}),
         ("box2", {"scale_div": 2})]


def make_cursor():
    """The synthetic source's 12x16 arrow, premultiplied ARGB."""
    c = np.zeros((16, 12), np.uint32)
    for y in range(16):
        for x in range(12):
            if x <= y and y < 14 - x // 3:
                edge = x == 0 or x == y or y == 13 - x // 3
                c[y, x] = 0xFF000000 if edge else 0xFFFFFFFF
    return c.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30,
                    help="timed frames per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", default="",
                    help="WxH[,WxH...] instead of 1080p and 4K")
    ap.add_argument("--markdown", action="store_true",
                    help="print the summary as a markdown table too")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_frontend: no HIP device is present")
    torch.cuda.set_device(0)
    torch.cuda.synchronize()

    import hipflux
    from hipflux import _native
    if hipflux.hip_device_count() == 0:
        sys.exit("bench_frontend: no HIP device is present")

    sizes = SIZES
    if args.sizes:
        sizes = [tuple(int(v) for v in s.split("x"))
                 for s in args.sizes.split(",")]
    cursor_img = make_cursor()
    rng = np.random.default_rng(1234)
    rows = []

    for (w, h) in sizes:
        # the frames outlive every front end below: pin_source may
        # page-lock them in place, as the engine does with capture buffers
        noise = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
                 for _ in range(4)]
        for mode, kw in MODES:
            for content in ("static", "noise"):
                gpu = _native.GpuFrontEnd(w, h, pin_source=True, **kw)
                cpu = _native._frontend_cpu(w, h, **kw)
                n_src = 1 if content == "static" else len(noise)

                def frame_args(i):
                    # the cursor rests on a static frame (nothing changes:
                    # the diff reads every block to the end) and moves
                    # over noise
                    k = 0 if content == "static" else i
                    cur = (cursor_img, 12, 16, (100 + 5 * k) % (w - 12),
                           (80 + 4 * k) % (h - 16))
                    return noise[i % n_src], cur

                def window(fe, first):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(first, first + args.steps):
                        f, cur = frame_args(i)
                        fe.process(f, w * 4, cursor=cur, threshold=15,
                                   duration=30, download=False)
                    return (time.perf_counter() - t0) * 1e3 / args.steps

                for fe in (cpu, gpu):
                    for i in range(args.warmup):
                        f, cur = frame_args(i)
                        fe.process(f, w * 4, cursor=cur, download=False)
                ms = {"host": [], "gpu": []}
                n = args.warmup
                for _ in range(args.repeats):
                    ms["host"].append(window(cpu, n))
                    ms["gpu"].append(window(gpu, n))
                    n += args.steps

                # stage breakdown from HIP events, untimed by the host
                gpu.set_timing(True)
                stages = {"h2d": [], "overlay": [], "scale": [],
                          "damage": []}
                for i in range(n, n + args.steps):
                    f, cur = frame_args(i)
                    r = gpu.process(f, w * 4, cursor=cur, threshold=15,
                                    duration=30, download=False)
                    for k, v in gpu.last_stage_ms().items():
                        stages[k].append(v)
                gpu.set_timing(False)
                ow, oh = r["w"], r["h"]
                st = {k: statistics.median(v) for k, v in stages.items()}

                native_b, scaled_b = w * h * 4, ow * oh * 4
                moved = {"damage": 2 * scaled_b}   # cur + prev, flags ~0
                if mode != "none":
                    moved["scale"] = native_b + scaled_b
                kern = {}
                for k, b in moved.items():
                    copy_ms = _native._d2d_copy_ms(b // 2, 20)
                    kern[k] = {"ms": round(st[k], 4),
                               "gbps": round(b / st[k] * 1e-6, 1),
                               "copy_ms": round(copy_ms, 4),
                               "copy_gbps": round(b / copy_ms * 1e-6, 1)}

                # what the host path still has to pay before the encoder
                # sees its frame: a pinned upload of the scaled frame
                t = torch.empty(scaled_b, dtype=torch.uint8).pin_memory()
                d = torch.empty(scaled_b, dtype=torch.uint8, device="cuda")
                ups = []
                for _ in range(10):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    d.copy_(t, non_blocking=True)
                    torch.cuda.synchronize()
                    ups.append((time.perf_counter() - t0) * 1e3)
                up_ms = statistics.median(ups)

                host, dev = statistics.median(ms["host"]), \
                    statistics.median(ms["gpu"])
                spread = max(max(ms["host"]) - min(ms["host"]),
                             max(ms["gpu"]) - min(ms["gpu"]))
                row = {
                    "size": f"{w}x{h}", "scale": mode, "content": content,
                    "host_ms": round(host, 3),
                    "host_min": round(min(ms["host"]), 3),
                    "host_max": round(max(ms["host"]), 3),
                    "gpu_ms": round(dev, 3),
                    "gpu_min": round(min(ms["gpu"]), 3),
                    "gpu_max": round(max(ms["gpu"]), 3),
                    "scaled_upload_ms": round(up_ms, 3),
                    "host_plus_upload_ms": round(host + up_ms, 3),
                    "gpu_slower_than_host": bool(dev - host > spread),
                    "stage_ms": {k: round(v, 4) for k, v in st.items()},
                    "kernels": kern,
                }
                rows.append(row)
                print(json.dumps(row), flush=True)
                del gpu, cpu, fe, t, d

    if args.markdown:
        print()
        print("| size | scale | content | host ms (min..max) | "
              "host+up ms | GPU ms (min..max) | h2d | overlay | scale "
              "(GB/s vs copy) | damage (GB/s vs copy) |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            def kcell(k):
                if k not in r["kernels"]:
                    return "-"
                v = r["kernels"][k]
                return (f"{v['ms']:.3f} ({v['gbps']:.0f} vs "
                        f"{v['copy_gbps']:.0f})")
            print(f"| {r['size']} | {r['scale']} | {r['content']} | "
                  f"{r['host_ms']:.2f} ({r['host_min']:.2f}.."
                  f"{r['host_max']:.2f}) | {r['host_plus_upload_ms']:.2f} | "
                  f"{r['gpu_ms']:.2f} ({r['gpu_min']:.2f}.."
                  f"{r['gpu_max']:.2f}) | {r['stage_ms']['h2d']:.3f} | "
                  f"{r['stage_ms']['overlay']:.3f} | {kcell('scale')} | "
                  f"{kcell('damage')} |")
    slow = [f"{r['size']} {r['scale']} {r['content']}" for r in rows
            if r["gpu_slower_than_host"]]
    print(json.dumps({"summary": {"configs": len(rows),
                                  "gpu_slower_than_host": slow}}))


if __name__ == "__main__":
    main()
