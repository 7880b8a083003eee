#!/usr/bin/env python3
"""Times the deep video path (include/srhip.h "Deep video") on 1920x1080 C420p10 frames (co-sited chroma), limited-range BT.709,
imagenet.rsr; one process, medians of hipEvent pairs.
  (a) sr_rgb_to_yuv16_dev of the 5760x3240 f32 image against the 8-bit sr_rgb_to_yuv_dev on the same tensor, alternating blocks: us,
      compulsory MB (every input byte read once, every output byte written once: 280 against 252), the fraction of the 6.3 TB/s HBM
      copy roof, the ratio of the two medians beside the ratio of their bytes, and the pair's run-to-run spread (the largest
      block median over the smallest, per kernel).
  (b) sr_yuv16_to_rgb_dev of the 1920x1080 frame against the 8-bit sr_yuv_to_rgb_dev, the same way.
  (c) sr_upscale_yuv16_dev against the plain sr_upscale_f32_dev of the same frame (as f32 RGB), alternating blocks, in exact f32 (the
      budget: 1.05) and in split-half.
  (d) The frame stream of sr_video_create16 in steady state, wall clock per frame over `--frames` frames, slots 3 and slots 1.
    python scripts/video_deep_bench.py [--reps N] [--frames N] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from border_bench import H, W, F, ROOF_GBPS, image, median, timed  # noqa: E402

BLOCKS = 6


def bench(reps, frames, out_path):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    fmt8 = r.YuvFormat.named("420", "left", "bt709", "limited")
    fmt = r.Yuv16Format.named("420", "left", "bt709", "limited", 10)
    fb8, ob8 = r.yuv_frame_bytes(fmt8, H, W), r.yuv_frame_bytes(fmt8, F * H, F * W)
    fb, ob = r.yuv16_frame_bytes(fmt, H, W), r.yuv16_frame_bytes(fmt, F * H, F * W)
    px = image()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    def pair(name, deep, eight, bytes_deep, bytes_eight, s):
        """Alternating blocks of the deep and the 8-bit launch: medians over all, and each kernel's spread over its block medians."""
        for _ in range(8):
            deep()
            eight()
        s.synchronize()
        td, te, md, me = [], [], [], []
        for _ in range(BLOCKS):
            a, b = timed(deep, s, reps), timed(eight, s, reps)
            td += a
            te += b
            md.append(median(a))
            me.append(median(b))
        d, e = median(td), median(te)
        emit({"pair": name, "size": f"{W}x{H}", "format": "420left bt709 limited, depth 10 against 8", "deep_us": round(1e3 * d, 2),
              "eight_us": round(1e3 * e, 2), "deep_MB": round(bytes_deep / 1e6, 1), "eight_MB": round(bytes_eight / 1e6, 1),
              "deep_frac_of_6.3TBps_copy_roof": round(bytes_deep / d / 1e6 / ROOF_GBPS, 4),
              "eight_frac_of_6.3TBps_copy_roof": round(bytes_eight / e / 1e6 / ROOF_GBPS, 4),
              "time_ratio": round(d / e, 4), "byte_ratio": round(bytes_deep / bytes_eight, 4),
              "deep_spread": round(max(md) / min(md), 4), "eight_spread": round(max(me) / min(me), 4), "reps": BLOCKS * reps})

    s = torch.cuda.Stream()
    for precision in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
        x = torch.from_numpy(px[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()
        d_frame = eng.rgb_to_yuv16_dev(x, fmt)               # the picture as a deep frame ...
        d_frame8 = eng.rgb_to_yuv_dev(x, fmt8)               # ... and as an 8-bit one
        d_rgb = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
        d_net = torch.empty((1, F * H, F * W, 3), dtype=torch.float32, device="cuda")
        d_out = torch.empty((1, ob // 2), dtype=torch.int16, device="cuda")
        d_out8 = torch.empty((1, ob8), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            eng.upscale_f32_dev(x, out=d_net, stream=s)      # a real output for the conversions to read
            if precision == "f32":                           # (the launches do not depend on the precision)
                pair("rgb_to_yuv16_vs_rgb2yuv", lambda: eng.rgb_to_yuv16_dev(d_net, fmt, out=d_out, stream=s),
                     lambda: eng.rgb_to_yuv_dev(d_net, fmt8, out=d_out8, stream=s), d_net.numel() * 4 + ob, d_net.numel() * 4 + ob8, s)
                pair("yuv16_to_rgb_vs_yuv2rgb", lambda: eng.yuv16_to_rgb_dev(d_frame, fmt, H, W, out=d_rgb, stream=s),
                     lambda: eng.yuv_to_rgb_dev(d_frame8, fmt8, H, W, out=d_rgb, stream=s), fb + d_rgb.numel() * 4, fb8 + d_rgb.numel() * 4, s)
            plain = lambda: eng.upscale_f32_dev(x, out=d_net, stream=s)
            video = lambda: eng.upscale_yuv16_dev(d_frame, fmt, H, W, out=d_out, stream=s)
            for _ in range(16):   # (the engine measures per shape whether a call runs as two bands: settled before anything is timed)
                plain()
                video()
            s.synchronize()
            t_plain, t_video = [], []
            for _ in range(4):
                t_plain += timed(plain, s, reps)
                t_video += timed(video, s, reps)
        p, v = median(t_plain), median(t_video)
        emit({"call": "yuv16_vs_plain_f32", "precision": precision, "size": f"{W}x{H}", "plain_ms": round(p, 4), "plain_min_ms": round(min(t_plain), 4),
              "yuv16_ms": round(v, 4), "yuv16_min_ms": round(min(t_video), 4), "ratio": round(v / p, 4),
              "ratio_min": round(min(t_video) / min(t_plain), 4), "reps": 4 * reps})
        frame = d_frame.cpu().numpy()[0].view(np.uint16)
        per = {}
        for slots in (3, 1):
            vs = r.VideoStream(eng, fmt, H, W, slots=slots)

            def run(count):   # the ring kept full; a received frame is looked at in place, as the CLI writes it from there
                for _ in range(count):
                    if vs.pending == slots:
                        vs.receive(copy=False)
                    vs.submit(frame)
                while vs.pending:
                    vs.receive(copy=False)
            run(8)
            t0 = time.perf_counter()
            run(frames)
            per[slots] = 1e3 * (time.perf_counter() - t0) / frames
            vs.close()
        emit({"call": "stream16", "precision": precision, "size": f"{W}x{H}", "frames": frames, "slots3_ms_per_frame": round(per[3], 4),
              "slots1_ms_per_frame": round(per[1], 4), "slots3_over_slots1": round(per[3] / per[1], 4), "kernels_ms": round(v, 4)})
        eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    bench(a.reps, a.frames, a.out)


if __name__ == "__main__":
    main()
