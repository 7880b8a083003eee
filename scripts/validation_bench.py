#!/usr/bin/env python3
"""Times the validation pass (include/srhip.h sr_validation_error_*) at factor 3 on u8 RGBA HR images of 1920x1080 and 3840x2160, in
both precisions:
  * call_ms   -- sr_validation_error_rgba8_dev (pool + network + loss + final sum), a hipEvent pair around it on its stream;
  * net_ms    -- the network alone on an LR image of the same size (sr_upscale_f32_dev, f32 output), the same way;
  * pool_loss -- call_ms - net_ms, and its share of the call;
  * host_ms   -- the synchronous host-pointer call (upload of the HR image included), wall clock, and its device time from
                 sr_last_timing with profiling on.
    python scripts/validation_bench.py [--reps N] [--out FILE.jsonl] [--size WxH] [--precision f32|split_f16]
    python scripts/validation_bench.py --summarize DIR     (the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of
                                                           this script: the pool / loss kernels' time, share and bandwidth)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1920, 1080), (3840, 2160))
COPY_TBPS = 6.29   # measured HBM copy rate of the MI355X (float4 copy)


def hr_image(w, h, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    # smooth content (the trained range of the bundled weights): a coarse random field, upsampled, plus a little noise
    small = rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 4)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=0), 16, axis=1)[:h, :w]
    big += rng.normal(0, 6, big.shape).astype(np.float32)
    return np.clip(big, 0, 255).astype(np.uint8)


def timed(fn, stream, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    stream.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def bench(reps, out_path, sizes=SIZES, precisions=("f32", "split_f16")):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    params = r.rsr.builtin("imagenet")
    rows = []
    for precision in precisions:
        eng = r.Engine(params, device=0, precision=precision)
        for w, h in sizes:
            hr = hr_image(w, h, w)
            s = torch.cuda.Stream()
            d_hr = torch.from_numpy(hr).cuda()
            res = torch.empty(1, dtype=torch.float64, device="cuda")
            lr = torch.rand((1, h // 3, w // 3, 3), device="cuda")
            out = torch.empty((1, h, w, 3), device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                call_ms, call_min = timed(lambda: eng.validation_error_dev(d_hr, out=res, stream=s), s, reps)
                net_ms, net_min = timed(lambda: eng.upscale_f32_dev(lr, out=out, stream=s), s, reps)
            eng.validation_error(hr)  # warm the host path
            walls = []
            for _ in range(max(3, reps // 4)):
                t = time.perf_counter()
                eng.validation_error(hr)
                walls.append((time.perf_counter() - t) * 1e3)
            eng.set_profiling(True)
            eng.validation_error(hr)
            host_dev_ms = eng.last_timing()["total_ms"]
            eng.set_profiling(False)
            row = {"precision": precision, "hr": f"{w}x{h}", "lr": f"{w // 3}x{h // 3}", "call_ms": round(call_ms, 4), "call_min_ms": round(call_min, 4),
                   "net_ms": round(net_ms, 4), "net_min_ms": round(net_min, 4), "pool_loss_ms": round(call_ms - net_ms, 4),
                   "pool_loss_share": round((call_ms - net_ms) / call_ms, 4), "host_wall_ms": round(sorted(walls)[len(walls) // 2], 3),
                   "host_device_ms": round(host_dev_ms, 3), "reps": reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
        eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def summarize(d):
    """Kernel times of a `rocprofv3 --kernel-trace --stats` run of this script (run with --reps small): the validation kernels'
    average time, and their bandwidth at the 4K HR shape (the loss kernel: f32 output + RGBA8 HR crop; the pool: RGBA8 HR + f32 LR)."""
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel_stats.csv under {d}")
    with open(files[0]) as f:
        stats = list(csv.DictReader(f))
    total = sum(float(s["TotalDurationNs"]) for s in stats)
    print(f"{'kernel':80s} {'calls':>6s} {'avg us':>9s} {'share':>7s}")
    for s in sorted(stats, key=lambda s: -float(s["TotalDurationNs"])):
        name = s["Name"]
        print(f"{name[:80]:80s} {int(s['Calls']):6d} {float(s['AverageNs']) / 1e3:9.2f} {float(s['TotalDurationNs']) / total:7.2%}")
    # per-call bytes at 4K (3840x2160 RGBA8 HR, 1280x720 LR) and 1080p
    for w, h in SIZES:
        px = w * h
        loss_b, pool_b = px * 12 + px * 4, px * 4 + (px // 9) * 12
        print(f"{w}x{h}: loss kernel moves {loss_b / 1e6:.1f} MB, pool {pool_b / 1e6:.1f} MB; at {COPY_TBPS} TB/s: {loss_b / COPY_TBPS / 1e6:.1f} us / "
              f"{pool_b / COPY_TBPS / 1e6:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--summarize", default="")
    ap.add_argument("--size", default="", help="WxH: this HR size only")
    ap.add_argument("--precision", default="", help="f32 | split_f16: this precision only")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else SIZES
        bench(a.reps, a.out, sizes, (a.precision,) if a.precision else ("f32", "split_f16"))


if __name__ == "__main__":
    main()
