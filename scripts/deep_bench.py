#!/usr/bin/env python3
"""Times the deep-colour path (include/srhip.h "Deep colour") on a 1920x1080 RGB16 image, imagenet.rsr, in both precisions.
  (a) The two conversion launches alone, a hipEvent pair around each on its stream: sr_u16_to_f32_dev of the 1920x1080 image (3 channels
      in) and sr_f32_to_u16_dev of the 5760x3240 f32 image (3, 4 and 1 channels out) -- us, GB/s of compulsory I/O (every input byte
      read once, every output byte written once) and its fraction of the 6.3 TB/s HBM copy roof scripts/video_bench.py uses; beside
      them sr_rgb_to_yuv_dev of the same f32 image, which moves a similar byte mix (profiles/video_bench.jsonl: 0.81 of the roof).
      The narrow form of f32_to_u16 (both pointers off their 16-byte boundary) is timed too: what an unaligned caller pays.
  (b) sr_upscale_u16_dev against the plain sr_upscale_f32_dev of the same picture (as f32 RGB), alternating blocks: the wrapper's
      ratio.  Exact f32 is held to 1.05, the budget of the alpha and resize paths; the split-half ratio is reported without a bar.
    python scripts/deep_bench.py [--reps N] [--out FILE.jsonl]     (one process; run it again for a repeat)
    python scripts/deep_bench.py --trace-run                       (the launches alone, for a kernel trace of their own)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from border_bench import H, W, F, ROOF_GBPS, image, median, timed  # noqa: E402

BUDGET_F32 = 1.05


def image16():
    """border_bench's picture promoted to 16 bits, with seeded low bytes"""
    import numpy as np
    px = image()[..., :3].astype(np.int64) * 257 + np.random.default_rng(16).integers(-128, 129, (H, W, 3))
    return np.clip(px, 0, 65535).astype(np.uint16)


def bench(reps, out_path):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    px = image16()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    s = torch.cuda.Stream()
    fmt = r.YuvFormat.named("420", "left", "bt709", "limited")
    for precision in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
        d_px = torch.from_numpy(px[None]).cuda()
        d_x = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
        d_net = torch.empty((1, F * H, F * W, 3), dtype=torch.float32, device="cuda")
        npx = F * H * F * W
        outs = {oc: torch.empty((1, F * H, F * W, oc), dtype=torch.uint16, device="cuda") for oc in (1, 3, 4)}
        d_yuv = torch.empty((1, r.yuv_frame_bytes(fmt, F * H, F * W)), dtype=torch.uint8, device="cuda")
        # the narrow form: an f32 image 4 bytes and a u16 image 2 bytes past a 16-byte boundary
        off_in = torch.empty((npx * 3 + 4,), dtype=torch.float32, device="cuda")
        off_out = torch.empty((npx * 3 + 8,), dtype=torch.uint16, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            eng.u16_to_f32_dev(d_px, out=d_x, stream=s)
            eng.upscale_f32_dev(d_x, out=d_net, stream=s)      # a real output for the conversions to read
            off_in[1:1 + npx * 3].copy_(d_net.reshape(-1))
            s.synchronize()
            narrow_in = off_in[1:1 + npx * 3].view(1, F * H, F * W, 3)
            narrow_out = off_out[1:1 + npx * 3].view(1, F * H, F * W, 3)
            assert narrow_in.data_ptr() % 16 == 4 and narrow_out.data_ptr() % 16 == 2
            launches = {
                "u16_to_f32 rgb": (lambda: eng.u16_to_f32_dev(d_px, out=d_x, stream=s), px.nbytes + d_x.numel() * 4),
                "f32_to_u16 rgb": (lambda: eng.f32_to_u16_dev(d_net, 3, out=outs[3], stream=s), npx * 12 + npx * 6),
                "f32_to_u16 rgba": (lambda: eng.f32_to_u16_dev(d_net, 4, out=outs[4], stream=s), npx * 12 + npx * 8),
                "f32_to_u16 grey": (lambda: eng.f32_to_u16_dev(d_net, 1, out=outs[1], stream=s), npx * 12 + npx * 2),
                "f32_to_u16 rgb narrow": (lambda: eng._L.sr_f32_to_u16_dev(eng._ctx, narrow_in.data_ptr(), 1, F * H, F * W, narrow_out.data_ptr(), 3,
                                                                          s.cuda_stream), npx * 12 + npx * 6),
                "rgb_to_yuv 420left": (lambda: eng.rgb_to_yuv_dev(d_net, fmt, out=d_yuv, stream=s), npx * 12 + d_yuv.numel()),
            }
            if precision == "f32":                             # (the launches do not depend on the precision)
                for name, (fn, compulsory) in launches.items():
                    for _ in range(8):
                        fn()
                    s.synchronize()
                    ts = timed(fn, s, 4 * reps)
                    med = median(ts)
                    emit({"launch": name, "us": round(1e3 * med, 2), "min_us": round(1e3 * min(ts), 2), "compulsory_MB": round(compulsory / 1e6, 1),
                          "compulsory_GBps": round(compulsory / med / 1e6, 1), "frac_of_6.3TBps_copy_roof": round(compulsory / med / 1e6 / ROOF_GBPS, 4),
                          "reps": 4 * reps})
                assert outs[3].cpu().numpy().tobytes() == narrow_out.cpu().numpy().tobytes()       # both forms, the same samples
            plain = lambda: eng.upscale_f32_dev(d_x, out=d_net, stream=s)
            deep = lambda: eng.upscale_u16_dev(d_px, 3, out=outs[3], stream=s)
            for _ in range(16):   # (the engine measures per shape whether a call runs as two bands: settled before anything is timed)
                plain()
                deep()
            s.synchronize()
            t_plain, t_deep = [], []
            for _ in range(4):
                t_plain += timed(plain, s, reps)
                t_deep += timed(deep, s, reps)
        p, v = median(t_plain), median(t_deep)
        row = {"call": "u16_vs_plain_f32", "precision": precision, "size": f"{W}x{H}", "plain_ms": round(p, 4), "plain_min_ms": round(min(t_plain), 4),
               "u16_ms": round(v, 4), "u16_min_ms": round(min(t_deep), 4), "ratio": round(v / p, 4), "ratio_min": round(min(t_deep) / min(t_plain), 4),
               "reps": 4 * reps}
        if precision == "f32":
            row["budget"] = BUDGET_F32
            row["within_budget"] = bool(v / p <= BUDGET_F32)
        emit(row)
        eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def trace_run():
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision="f32")
    d_px = torch.from_numpy(image16()[None]).cuda()
    d_net = torch.rand((1, F * H, F * W, 3), dtype=torch.float32, device="cuda")
    for _ in range(6):
        eng.u16_to_f32_dev(d_px)
        for oc in (3, 4, 1):
            eng.f32_to_u16_dev(d_net, oc)
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
