#!/usr/bin/env python3
"""The workload of the kernel-by-name comparison of video at any size: the 5760x3240 f32 output of a 1080p frame ->
3840x2160, lanczos3, to a frame of every format class -- 8-bit 4:2:0 centre / left and 4:4:4, 10-bit 4:2:0 and 4:2:2 under both sitings
and 4:4:4 -- `--reps` times the fused kernel (sr_resize_to_yuv[16] under "vyuv" = --pairs: resize_v_yuv_kernel) and the chain on the same
input (sr_resize_dev f32 -> f32: resize_v_kernel, then sr_rgb_to_yuv[16]_dev: rgb_to_yuv_kernel).  The kernels' names carry the class
(sample type, subsampling, siting), so the profiler's statistics by name are the comparison: the rule of sr_yuv.cpp fused_pays is read
off them.  Run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python scripts/video_sized_rocprof.py [--reps 5] [--pairs 1|2]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    import numpy as np
    import torch
    import rusty_sr_amd as r
    from border_bench import image
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", default="2")
    a = ap.parse_args()
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0)
    eng.set_experiment("vyuv", a.pairs)
    x = torch.from_numpy(image()[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()
    d_net = eng.upscale_f32_dev(x)
    torch.cuda.synchronize()
    net = d_net.cpu().numpy()
    fmts = [("yuv", r.YuvFormat.named(sub, siting, "bt709", "limited")) for sub, siting in (("420", "center"), ("420", "left"), ("444", "center"))]
    fmts += [("yuv16", r.Yuv16Format.named(sub, siting, "bt709", "limited", 10))
             for sub, siting in (("420", "center"), ("420", "left"), ("422", "center"), ("422", "left"), ("444", "center"))]
    for tag, fmt in fmts:
        for _ in range(a.reps):
            fused = getattr(eng, f"resize_to_{tag}")(net, fmt, (2160, 3840))
            res = eng.resize_dev(d_net, (2160, 3840), "f32")
            chain = getattr(eng, f"rgb_to_{tag}_dev")(res, fmt)
            torch.cuda.synchronize()
        assert fused.tobytes() == chain.cpu().numpy().tobytes(), tag
    print("fused == chain on every format class")


if __name__ == "__main__":
    main()
