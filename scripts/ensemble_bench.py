#!/usr/bin/env python3
"""Times the self-ensemble (include/srhip.h sr_upscale_ensemble_rgba8_dev) on u8 RGB images of 1920x1080 and 640x480, RGBA8 out,
imagenet.rsr, exact f32, a hipEvent pair around each call on its stream:
  * ens_ms      -- the ensemble call with masks 0xFF and 0x0F;
  * base_ms     -- in the same process, the plain calls it is made of, one timed region: 4 at h x w and 4 at w x h for 0xFF, 4 at h x w
                   for 0x0F (sr_upscale_f32_dev: a member's pass writes f32);
  * ratio       -- ens_ms / base_ms: what the pixel moves (input transform, accumulate) add to the passes;
  * plain_ms    -- one plain sr_upscale_rgba8_dev call (the flagship call; compared across builds with --plain-only, see below).
    python scripts/ensemble_bench.py [--reps N] [--out FILE.jsonl]
    python scripts/ensemble_bench.py --plain-only [--reps N]      (one JSON line: the plain 1080p call's median; run in three fresh
                                                                  processes on each of two builds to compare them)
    python scripts/ensemble_bench.py --summarize DIR              (the kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run of
                                                                  `--trace-run`: the ens_* launches' time and bandwidth at 1080p)"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((1920, 1080), (640, 480))
COPY_TBPS = 6.29   # measured HBM copy rate of the MI355X (float4 copy)


def image(w, h, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=0), 16, axis=1)[:h, :w]
    big += rng.normal(0, 6, big.shape).astype(np.float32)
    return np.clip(big, 0, 255).astype(np.uint8)


def timed(fn, stream, reps, warmup=5):
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


def bench(reps, out_path, sizes=SIZES, plain_only=False):
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    rows = []
    for w, h in sizes:
        px = image(w, h, w)
        s = torch.cuda.Stream()
        d_px = torch.from_numpy(px[None]).cuda()
        d_pt = d_px.transpose(1, 2).contiguous()
        d_x, d_xt = d_px.float() / 255, d_pt.float() / 255
        out8 = torch.empty((1, 3 * h, 3 * w, 4), dtype=torch.uint8, device="cuda")
        out, out_t = torch.empty((1, 3 * h, 3 * w, 3), device="cuda"), torch.empty((1, 3 * w, 3 * h, 3), device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            # (the engine measures per shape whether a call runs as two bands: 16 calls of each shape settle that before anything is timed)
            for _ in range(16):
                eng.upscale_rgba8_dev(d_px, out=out8, stream=s)
                eng.upscale_f32_dev(d_x, out=out, stream=s)
                eng.upscale_f32_dev(d_xt, out=out_t, stream=s)
            s.synchronize()
            plain_ms, plain_min = timed(lambda: eng.upscale_rgba8_dev(d_px, out=out8, stream=s), s, reps)
            row = {"size": f"{w}x{h}", "plain_ms": round(plain_ms, 4), "plain_min_ms": round(plain_min, 4), "reps": reps}
            if not plain_only:
                def base(n_hw, n_wh):
                    for _ in range(n_hw):
                        eng.upscale_f32_dev(d_x, out=out, stream=s)
                    for _ in range(n_wh):
                        eng.upscale_f32_dev(d_xt, out=out_t, stream=s)
                for mask, (n_hw, n_wh) in ((0xFF, (4, 4)), (0x0F, (4, 0))):
                    ens_ms, ens_min = timed(lambda: eng.upscale_ensemble_rgba8_dev(d_px, members=mask, out=out8, stream=s), s, reps)
                    base_ms, base_min = timed(lambda: base(n_hw, n_wh), s, reps)
                    tag = f"{mask:#04x}"
                    row.update({f"ens_{tag}_ms": round(ens_ms, 4), f"ens_{tag}_min_ms": round(ens_min, 4), f"base_{tag}_ms": round(base_ms, 4),
                                f"base_{tag}_min_ms": round(base_min, 4), f"ratio_{tag}": round(ens_ms / base_ms, 4)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def trace_run():
    """What a `rocprofv3 --kernel-trace --stats` run traces: a few ensemble calls of all 8 members at 1080p, RGBA8 and f32 output."""
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    w, h = SIZES[0]
    d_px = torch.from_numpy(image(w, h, w)[None]).cuda()
    for _ in range(6):
        eng.upscale_ensemble_rgba8_dev(d_px, members=0xFF)
        eng.upscale_ensemble_f32_dev(d_px.float() / 255, members=0xFF)
    torch.cuda.synchronize()
    eng.close()


def summarize(d):
    """The ens_* kernels of such a run, launch by launch, from its kernel_trace.csv: the accumulate launches of a call come in the order of
    its 8 members, and what one moves per output pixel depends on its place -- it reads the member's map (12 B); all but the first read
    the accumulator (12 B); all but the last write it (12 B), the last writes the output (4 B RGBA8, 12 B f32).  The input transforms
    read 3 B (u8 RGB) or 12 B (f32) and write 12 B per input pixel.  Per kind of launch: the median time and those bytes over it."""
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel_trace.csv under {d}")
    with open(files[0]) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    w, h = SIZES[0]
    in_px, out_px = w * h, 9 * w * h
    kinds, seen = {}, {}
    for r in rows:
        name = r["Kernel_Name"]
        if "ens_" not in name:
            continue
        ns = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        form = "tile" if "ens_tile" in name else "rows"
        if "SinkAcc" in name:
            u8 = "SinkAcc<true>" in name or "SinkAccILb1" in name  # (demangled or not)
            i = seen.get(u8, 0)  # the calls of either output form are whole runs of 8 accumulate launches
            seen[u8] = i + 1
            place = "first" if i % 8 == 0 else "last" if i % 8 == 7 else "middle"
            per_px = 12 + (0 if place == "first" else 12) + (12 if place != "last" else 4 if u8 else 12)
            key, nbytes = f"accumulate {form} {place} ({'rgba8' if u8 else 'f32'} call), {per_px} B/px", out_px * per_px
        else:
            f32 = "SrcF32" in name
            key, nbytes = f"input {form} ({'f32' if f32 else 'u8 rgb'}), {24 if f32 else 15} B/px", in_px * (24 if f32 else 15)
        kinds.setdefault(key, (nbytes, []))[1].append(ns)
    print(f"{'launch':64s} {'n':>4s} {'median us':>10s} {'min us':>8s} {'GB/s':>8s}")
    for key, (nbytes, t) in sorted(kinds.items()):
        t.sort()
        med = t[len(t) // 2]
        print(f"{key:64s} {len(t):4d} {med / 1e3:10.2f} {t[0] / 1e3:8.2f} {nbytes / med:8.0f}")
    print(f"HBM copy rate for comparison: {COPY_TBPS * 1e3:.0f} GB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default="")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarize", default="")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.trace_run:
        trace_run()
    else:
        bench(a.reps, a.out, SIZES[:1] if a.plain_only else SIZES, a.plain_only)


if __name__ == "__main__":
    main()
