#!/usr/bin/env python3
"""Times the border modes (include/srhip.h "Borders") on 1920x1080 images, imagenet.rsr, exact f32, a hipEvent pair around each call on
its stream.
  * The two launches alone, RGBA8 and f32: the pad of the 1920x1080 image by 8 (sr_pad_*_dev) and the crop of the centre 5760x3240 out
    of the 5808x3288 output of the padded image (sr_crop_*_dev) -- ms, GB/s of compulsory I/O (every output byte written once and read
    once) and its fraction of the 6.3 TB/s HBM copy roof, the yardstick of sr_aux.hip's copy-like kernels.
  * The composed call against the plain call of the same image, RGBA8 and f32, in alternating blocks: plain_ms (sr_upscale_*_dev),
    border_ms (sr_upscale_*_border_dev, wrap, pad 8, members 1), ratio, and area -- (h + 16)(w + 16) / (h w), the share of the ratio
    that is the network running on more pixels; ratio / area is what the two copies add on top.
    python scripts/border_bench.py [--reps N] [--out FILE.jsonl]     (one process; run it three times for three repeats)
    python scripts/border_bench.py --trace-run                       (what a `rocprofv3 --kernel-trace --stats` run traces)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, PAD, F = 1920, 1080, 8, 3
ROOF_GBPS = 6300.0


def image(seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=0), 16, axis=1)[:H, :W]
    big += rng.normal(0, 6, big.shape).astype(np.float32)
    px = np.empty((H, W, 4), np.uint8)
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


def median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def bench(reps, out_path):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    px = image()
    rows = []
    s = torch.cuda.Stream()
    for io in ("rgba8", "f32"):
        u8 = io == "rgba8"
        d_in = torch.from_numpy(px[None] if u8 else (px[None, ..., :3].astype(np.float32) / np.float32(255))).cuda()
        ch, dt, item = (4, torch.uint8, 1) if u8 else (3, torch.float32, 4)
        d_pad = torch.empty((1, H + 2 * PAD, W + 2 * PAD, ch), dtype=dt, device="cuda")
        d_big = torch.empty((1, F * (H + 2 * PAD), F * (W + 2 * PAD), ch), dtype=dt, device="cuda")
        d_out = torch.empty((1, F * H, F * W, ch), dtype=dt, device="cuda")
        d_big.copy_(torch.randint(0, 255, d_big.shape, device="cuda").to(dt))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            launches = {
                "pad": (lambda: eng.pad(d_in, "wrap", PAD, out=d_pad, stream=s), 2 * d_pad.numel() * item),
                "crop": (lambda: eng.crop(d_big, F * PAD, F * PAD, F * H, F * W, out=d_out, stream=s), 2 * d_out.numel() * item),
            }
            for name, (fn, compulsory) in launches.items():
                for _ in range(8):
                    fn()
                s.synchronize()
                ts = timed(fn, s, 4 * reps)
                med = median(ts)
                row = {"launch": name, "io": io, "size": f"{W}x{H}", "pad": PAD, "ms": round(med, 5), "min_ms": round(min(ts), 5),
                       "compulsory_GBps": round(compulsory / med / 1e6, 1), "frac_of_6.3TBps_copy_roof": round(compulsory / med / 1e6 / ROOF_GBPS, 4),
                       "reps": 4 * reps}
                print(json.dumps(row), flush=True)
                rows.append(row)
            if u8:
                plain = lambda: eng.upscale_rgba8_dev(d_in, out=d_out, stream=s)
                border = lambda: eng.upscale_rgba8_border_dev(d_in, "wrap", PAD, out=d_out, stream=s)
            else:
                plain = lambda: eng.upscale_f32_dev(d_in, out=d_out, stream=s)
                border = lambda: eng.upscale_f32_border_dev(d_in, "wrap", PAD, out=d_out, stream=s)
            # (the engine measures per shape whether a call runs as two bands: 16 calls of each kind settle that before anything is timed)
            for _ in range(16):
                plain()
                border()
            s.synchronize()
            t_plain, t_border = [], []
            for _ in range(4):  # alternating blocks
                t_plain += timed(plain, s, reps)
                t_border += timed(border, s, reps)
        p, b = median(t_plain), median(t_border)
        area = (H + 2 * PAD) * (W + 2 * PAD) / (H * W)
        row = {"call": "border_vs_plain", "io": io, "size": f"{W}x{H}", "pad": PAD, "plain_ms": round(p, 4), "plain_min_ms": round(min(t_plain), 4),
               "border_ms": round(b, 4), "border_min_ms": round(min(t_border), 4), "ratio": round(b / p, 4),
               "ratio_min": round(min(t_border) / min(t_plain), 4), "area": round(area, 4), "ratio_over_area": round(b / p / area, 4),
               "reps": 4 * reps}
        print(json.dumps(row), flush=True)
        rows.append(row)
    eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def trace_run():
    import numpy as np
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    px = image()
    for d_in in (torch.from_numpy(px[None]).cuda(), torch.from_numpy(px[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()):
        big = torch.zeros((1, F * (H + 2 * PAD), F * (W + 2 * PAD), d_in.shape[-1]), dtype=d_in.dtype, device="cuda")
        for _ in range(6):
            eng.pad(d_in, "wrap", PAD)
            eng.crop(big, F * PAD, F * PAD, F * H, F * W)
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
