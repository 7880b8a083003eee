#!/usr/bin/env python3
"""Times the transparency path (include/srhip.h sr_upscale_rgba8_alpha_dev) against the plain call of the same build on 1920x1080 RGBA8
images, imagenet.rsr, exact f32, a hipEvent pair around each call on its stream.  Two images: all opaque (the bleed copies its tiles
straight through) and half transparent (the left half of every 64-pixel column band visible, so that every bleed tile has work to do).
Per image, plain and alpha calls are timed in alternating blocks:
  * plain_ms  -- sr_upscale_rgba8_dev on the RGBA image (alpha dropped);
  * alpha_ms  -- sr_upscale_rgba8_alpha_dev, bleed 8, members 1: bleed + the same network pass + merge;
  * ratio     -- alpha_ms / plain_ms (the budget of DESIGN.md 4m: 1.05).
    python scripts/alpha_bench.py [--reps N] [--out FILE.jsonl]     (one process; run it three times for three repeats)
    python scripts/alpha_bench.py --trace-run                       (what a `rocprofv3 --kernel-trace --stats` run traces)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 1920, 1080


def image(kind, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=0), 16, axis=1)[:H, :W]
    big += rng.normal(0, 6, big.shape).astype(np.float32)
    px = np.empty((H, W, 4), np.uint8)
    px[..., :3] = np.clip(big, 0, 255).astype(np.uint8)
    px[..., 3] = 255
    if kind == "half":
        clear = (np.arange(W) % 64) >= 32
        px[:, clear, 3] = 0
        px[:, clear, :3] = 0
    return px


def timed(fn, stream, reps):
    import torch
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def bench(reps, out_path):
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    rows = []
    for kind in ("opaque", "half"):
        s = torch.cuda.Stream()
        d_px = torch.from_numpy(image(kind)[None]).cuda()
        out8 = torch.empty((1, 3 * H, 3 * W, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            plain = lambda: eng.upscale_rgba8_dev(d_px, out=out8, stream=s)
            alpha = lambda: eng.upscale_rgba8_alpha_dev(d_px, bleed=8, members=1, out=out8, stream=s)
            # (the engine measures per shape whether a call runs as two bands: 16 calls of each kind settle that before anything is timed)
            for _ in range(16):
                plain()
                alpha()
            s.synchronize()
            t_plain, t_alpha = [], []
            for _ in range(4):  # alternating blocks
                t_plain += timed(plain, s, reps)
                t_alpha += timed(alpha, s, reps)
        t_plain.sort()
        t_alpha.sort()
        p, a = t_plain[len(t_plain) // 2], t_alpha[len(t_alpha) // 2]
        row = {"image": kind, "size": f"{W}x{H}", "plain_ms": round(p, 4), "plain_min_ms": round(t_plain[0], 4), "alpha_ms": round(a, 4),
               "alpha_min_ms": round(t_alpha[0], 4), "ratio": round(a / p, 4), "ratio_min": round(t_alpha[0] / t_plain[0], 4),
               "reps": 4 * reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def trace_run():
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    for kind in ("opaque", "half"):
        d_px = torch.from_numpy(image(kind)[None]).cuda()
        for _ in range(6):
            eng.upscale_rgba8_alpha_dev(d_px, bleed=8)
        torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
    else:
        bench(a.reps, a.out)


if __name__ == "__main__":
    main()
