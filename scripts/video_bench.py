#!/usr/bin/env python3
"""Times the video path (include/srhip.h "Video") on 1920x1080 C420mpeg2 frames, limited-range BT.709, imagenet.rsr, in both precisions.
  (a) The two conversion launches alone, a hipEvent pair around each on its stream: sr_yuv_to_rgb_dev of the 1920x1080 frame and
      sr_rgb_to_yuv_dev of the 5760x3240 f32 image -- us, GB/s of compulsory I/O (every input byte read once, every output byte written
      once) and its fraction of the 6.3 TB/s HBM copy roof; the yardstick is the f32 crop's 0.84-0.92.
  (b) sr_upscale_yuv_dev against the plain sr_upscale_f32_dev of the same frame (as f32 RGB), alternating blocks: the wrapper's ratio.
  (c) The frame stream in steady state, wall clock per frame over `--frames` frames: slots 3, slots 1, and a loop of the plain host call
      sr_upscale_rgba8 on the same picture as RGB with a page-locked output (what a caller without the stream would run), with the
      device time of one frame's kernels and of its download beside them: how far ms/frame sits above the larger of the two.
    python scripts/video_bench.py [--reps N] [--frames N] [--out FILE.jsonl]     (one process; run it again for a repeat)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from border_bench import H, W, F, ROOF_GBPS, image, median, timed  # noqa: E402


def bench(reps, frames, out_path):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    fmt = r.YuvFormat.named("420", "left", "bt709", "limited")
    fb, ob = r.yuv_frame_bytes(fmt, H, W), r.yuv_frame_bytes(fmt, F * H, F * W)
    px = image()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    s = torch.cuda.Stream()
    for precision in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
        x = torch.from_numpy(px[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()
        d_frame = eng.rgb_to_yuv_dev(x, fmt)                 # the picture as a frame
        d_rgb = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
        d_net = torch.empty((1, F * H, F * W, 3), dtype=torch.float32, device="cuda")
        d_out = torch.empty((1, ob), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            eng.upscale_f32_dev(x, out=d_net, stream=s)      # a real output for the conversion to read
            launches = {
                "yuv2rgb": (lambda: eng.yuv_to_rgb_dev(d_frame, fmt, H, W, out=d_rgb, stream=s), fb + d_rgb.numel() * 4),
                "rgb2yuv": (lambda: eng.rgb_to_yuv_dev(d_net, fmt, out=d_out, stream=s), d_net.numel() * 4 + ob),
            }
            if precision == "f32":                           # (the launches do not depend on the precision)
                for name, (fn, compulsory) in launches.items():
                    for _ in range(8):
                        fn()
                    s.synchronize()
                    ts = timed(fn, s, 4 * reps)
                    med = median(ts)
                    emit({"launch": name, "size": f"{W}x{H}", "format": "420left bt709 limited", "us": round(1e3 * med, 2),
                          "min_us": round(1e3 * min(ts), 2), "compulsory_MB": round(compulsory / 1e6, 1),
                          "compulsory_GBps": round(compulsory / med / 1e6, 1), "frac_of_6.3TBps_copy_roof": round(compulsory / med / 1e6 / ROOF_GBPS, 4),
                          "reps": 4 * reps})
            plain = lambda: eng.upscale_f32_dev(x, out=d_net, stream=s)
            video = lambda: eng.upscale_yuv_dev(d_frame, fmt, H, W, out=d_out, stream=s)
            for _ in range(16):   # (the engine measures per shape whether a call runs as two bands: settled before anything is timed)
                plain()
                video()
            s.synchronize()
            t_plain, t_video = [], []
            for _ in range(4):
                t_plain += timed(plain, s, reps)
                t_video += timed(video, s, reps)
        p, v = median(t_plain), median(t_video)
        emit({"call": "yuv_vs_plain_f32", "precision": precision, "size": f"{W}x{H}", "plain_ms": round(p, 4), "plain_min_ms": round(min(t_plain), 4),
              "yuv_ms": round(v, 4), "yuv_min_ms": round(min(t_video), 4), "ratio": round(v / p, 4), "ratio_min": round(min(t_video) / min(t_plain), 4),
              "reps": 4 * reps})
        # (c) the stream
        frame = d_frame.cpu().numpy()[0]
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
        out8 = r.engine.host_alloc((1, F * H, F * W, 4))
        rgb = np.ascontiguousarray(px[None, ..., :3])
        for _ in range(4):
            eng.upscale_rgba8(rgb, out=out8.array)
        t0 = time.perf_counter()
        for _ in range(frames):
            eng.upscale_rgba8(rgb, out=out8.array)
        host = 1e3 * (time.perf_counter() - t0) / frames
        out8.close()
        # one frame's download alone, from device memory to a page-locked buffer
        pin = torch.empty((ob,), dtype=torch.uint8).pin_memory()
        with torch.cuda.stream(s):
            t_down = timed(lambda: pin.copy_(d_out[0], non_blocking=True), s, 2 * reps)
        down = median(t_down)
        emit({"call": "stream", "precision": precision, "size": f"{W}x{H}", "frames": frames, "slots3_ms_per_frame": round(per[3], 4),
              "slots1_ms_per_frame": round(per[1], 4), "host_rgba8_loop_ms_per_frame": round(host, 4), "slots3_over_slots1": round(per[3] / per[1], 4),
              "slots3_over_host_rgba8": round(per[3] / host, 4), "kernels_ms": round(v, 4), "download_ms": round(down, 4),
              "slots3_over_max_of_kernels_and_download": round(per[3] / max(v, down), 4)})
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
