#!/usr/bin/env python3
"""Times the resampling to any size (include/srhip.h "Resampling to any size") on device-resident images, a hipEvent pair around each
call on its stream, and appends one JSON line per row to profiles/resize_bench.jsonl (or --out).
  passes  sr_resize_dev alone (tap kernel + horizontal + vertical pass): 5760x3240 -> 3840x2160 and -> 1920x1080, f32 -> RGBA8 and
          RGBA8 -> RGBA8, lanczos3 and box.  All eight cases are warmed, then timed in interleaved rounds (every round times each case
          once, a block of --reps calls).  Reported: the median call, the fastest, the 10th-90th percentile spread, and the rate as a
          fraction of the 6.3 TB/s copy roof -- of the compulsory I/O (input once + output once), as the bilinear
          and downsample graphs are reported, and of the bytes the two passes really move (the f32 intermediate written and read too).
  sized   sr_upscale_rgba8_sized_dev, 1920x1080 -> 3840x2160, lanczos3, against sr_upscale_rgba8_dev of the same build on the same
          image (which writes 5760x3240), in alternating blocks, in both precisions: the ratio of the medians, and the spread of the
          per-round ratios.
    python scripts/resize_bench.py [--reps N] [--rounds N] [--out FILE.jsonl]
    python scripts/resize_bench.py --trace-run        (what a `rocprofv3 --kernel-trace --stats` run traces: a few calls of each pass case)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC_H, SRC_W = 3240, 5760
TARGETS = ((2160, 3840), (1080, 1920))
ROOF_GBPS = 6300.0


def picture(h, w, seed=7):
    """A blocky picture with noise on it, RGBA8 (alpha 255)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (h // 16 + 2, w // 16 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=0), 16, axis=1)[:h, :w]
    big += rng.normal(0, 6, big.shape).astype(np.float32)
    px = np.empty((h, w, 4), np.uint8)
    px[..., :3] = np.clip(big, 0, 255).astype(np.uint8)
    px[..., 3] = 255
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


def pct(sorted_times, q):
    return sorted_times[min(len(sorted_times) - 1, int(q * len(sorted_times)))]


def pass_cases(eng, torch, s):
    px = picture(SRC_H, SRC_W)
    d_u8 = torch.from_numpy(px[None]).cuda()
    d_f32 = (d_u8[..., :3].to(torch.float32) / 255.0).contiguous()
    cases = []
    for oh, ow in TARGETS:
        out8 = torch.empty((1, oh, ow, 4), dtype=torch.uint8, device="cuda")
        for io, src in (("f32->rgba8", d_f32), ("rgba8->rgba8", d_u8)):
            for flt in ("lanczos3", "box"):
                in_bytes = SRC_H * SRC_W * (12 if src is d_f32 else 4)
                mid_bytes = SRC_H * ow * 12
                cases.append({"io": io, "filter": flt, "to": f"{ow}x{oh}", "compulsory": in_bytes + oh * ow * 4,
                              "moved": in_bytes + 2 * mid_bytes + oh * ow * 4,
                              "fn": (lambda src=src, out8=out8, oh=oh, ow=ow, flt=flt: eng.resize_dev(src, (oh, ow), "rgba8", flt, out=out8, stream=s))})
    return cases


def bench_passes(eng, torch, reps, rounds):
    s = torch.cuda.Stream()
    rows = []
    with torch.cuda.stream(s):
        cases = pass_cases(eng, torch, s)
        torch.cuda.synchronize()
        for c in cases:  # warm every shape the timed window uses (the workspace grows here)
            for _ in range(5):
                c["fn"]()
        s.synchronize()
        times = [[] for _ in cases]
        for _ in range(rounds):  # interleaved: every round times each case once
            for k, c in enumerate(cases):
                times[k] += timed(c["fn"], s, reps)
    for c, t in zip(cases, times):
        t.sort()
        med = t[len(t) // 2]
        rows.append({"bench": "passes", "from": f"{SRC_W}x{SRC_H}", "to": c["to"], "io": c["io"], "filter": c["filter"], "ms": round(med, 4),
                     "min_ms": round(t[0], 4), "p10_ms": round(pct(t, 0.1), 4), "p90_ms": round(pct(t, 0.9), 4), "calls": len(t),
                     "compulsory_GBps": round(c["compulsory"] / med / 1e6, 1), "frac_of_6.3TBps_copy_roof": round(c["compulsory"] / med / 1e6 / ROOF_GBPS, 4),
                     "moved_GBps": round(c["moved"] / med / 1e6, 1), "moved_frac_of_copy_roof": round(c["moved"] / med / 1e6 / ROOF_GBPS, 4)})
    return rows


def bench_sized(r, torch, reps, rounds):
    H, W, OH, OW = 1080, 1920, 2160, 3840
    rows = []
    for prec in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=prec)
        s = torch.cuda.Stream()
        d_px = torch.from_numpy(picture(H, W)[None]).cuda()
        plain_out = torch.empty((1, 3 * H, 3 * W, 4), dtype=torch.uint8, device="cuda")
        sized_out = torch.empty((1, OH, OW, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            plain = lambda: eng.upscale_rgba8_dev(d_px, out=plain_out, stream=s)
            sized = lambda: eng.upscale_rgba8_sized_dev(d_px, (OH, OW), "lanczos3", out=sized_out, stream=s)
            # (the engine measures per shape whether a call runs as two bands: 16 calls of each kind settle that before anything is timed)
            for _ in range(16):
                plain()
                sized()
            s.synchronize()
            t_plain, t_sized, ratios = [], [], []
            for _ in range(rounds):  # alternating blocks
                a, b = sorted(timed(plain, s, reps)), sorted(timed(sized, s, reps))
                ratios.append(b[len(b) // 2] / a[len(a) // 2])
                t_plain += a
                t_sized += b
        t_plain.sort()
        t_sized.sort()
        p, z = t_plain[len(t_plain) // 2], t_sized[len(t_sized) // 2]
        rows.append({"bench": "sized", "precision": prec, "from": f"{W}x{H}", "to": f"{OW}x{OH}", "filter": "lanczos3", "plain_ms": round(p, 4),
                     "plain_min_ms": round(t_plain[0], 4), "sized_ms": round(z, 4), "sized_min_ms": round(t_sized[0], 4), "ratio": round(z / p, 4),
                     "ratio_rounds_min": round(min(ratios), 4), "ratio_rounds_max": round(max(ratios), 4), "calls": len(t_plain)})
        eng.close()
    return rows


def trace_run():
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(graph="bilinear")
    s = torch.cuda.current_stream()
    for c in pass_cases(eng, torch, s):
        for _ in range(6):
            c["fn"]()
        torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_bench.jsonl"))
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    if a.trace_run:
        trace_run()
        return
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(graph="bilinear")  # any context resamples: no parameters are used
    rows = bench_passes(eng, torch, a.reps, a.rounds)
    eng.close()
    rows += bench_sized(r, torch, a.reps, a.rounds)
    with open(a.out, "a") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
