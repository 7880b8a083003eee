#!/usr/bin/env python3
"""Times backpropagation (include/srhip.h sr_backprop_rgba8_dev) at factor 3 on u8 RGB HR batches, against the same step through
torch autograd (f32, same device), measured in the same run:
  * call_ms    -- sr_backprop_rgba8_dev (pool, forward with saved state, loss, data and weight gradients, assembly), a hipEvent pair
                  around it on its stream, median after warm-up;
  * torch_ms   -- pool, forward, loss and loss.backward() of the same graph in torch (channels_last f32 convolutions), the same way;
  * tflops     -- 2 x (forward + data-gradient + weight-gradient MACs) per LR pixel x LR pixels / call_ms, and its share of the
                  157.3 TF f32-MFMA peak;
  * launches   -- kernel launches per call (sr_grad.hip header).
    python scripts/backprop_bench.py [--reps N] [--out FILE.jsonl] [--no-torch]
    python scripts/backprop_bench.py --summarize DIR   (the database of a `rocprofv3 --kernel-trace --stats` run of this script with
                                                        --reps 5 --no-torch: time per kernel, and the conv kernels' share of peak)"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("reference_step", 4, 192, 192), ("large_batch", 16, 384, 384))
PEAK_TF = 157.3
E3 = 27
FWD_MACS = 2400 + 3 * 25600 + 3 * 9216 + 3 * E3 * 288   # 130 176 per LR pixel at f = 3
DGRAD_MACS = FWD_MACS - 2400                              # no data gradient into the input
WGRAD_MACS = FWD_MACS


def flops_per_call(n, h, w, f=3):
    return 2.0 * (FWD_MACS + DGRAD_MACS + WGRAD_MACS) * n * (h // f) * (w // f)


def hr_batch(n, h, w, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (n, h // 16 + 2, w // 16 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(small, 16, axis=1), 16, axis=2)[:, :h, :w]
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


def torch_step(params, hr_u8, f=3):
    """The training step in torch autograd, f32 on the device: returns a closure that runs pool + forward + loss + backward."""
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import grad_ref
    dev = hr_u8.device
    p = torch.tensor(params, dtype=torch.float32, device=dev, requires_grad=True)
    S = grad_ref.segments(f)
    hr = hr_u8[..., :3].float() / 255.0
    n, h, w, _ = hr.shape
    th = float(grad_ref.THRESH)

    def s2l(x):
        return torch.where(x <= th, x / 12.92, ((torch.clamp(x, min=0.04) + 0.055) / 1.055) ** 2.4)

    def l2s(v):
        return torch.where(v <= 0.0031308, 12.92 * v, 1.055 * torch.clamp(v, min=0.0031) ** (1 / 2.4) - 0.055)

    def step():
        g = {k: p[o:o + m].reshape(shape) for k, (o, m, shape) in S.items()}
        tgt = hr[:, :f * (h // f), :f * (w // f)]
        x = l2s(F.avg_pool2d(s2l(tgt).permute(0, 3, 1, 2), f)).contiguous(memory_format=torch.channels_last)

        def conv(t, k):
            wt = g[k].permute(0, 3, 1, 2)
            return F.conv2d(t, wt, padding=wt.shape[-1] // 2)

        def b(k):
            return g[k].reshape(1, -1, 1, 1)

        def belu(z, beta):
            return beta * z + torch.sqrt(z * z + 1.0) - 1.0
        a0 = belu(conv(x, "conv0") + b("f_bias"), b("f_activ"))
        a1 = belu(conv(a0, "conv1") + b("l1_bias"), b("l1_activ"))
        a2 = belu(conv(a0, "conv2") + b("l2_bias") + conv(a1, "conv5"), b("l2_activ"))
        a3 = belu(conv(a0, "conv3") + b("l3_bias") + conv(a1, "conv6") + conv(a2, "conv8"), b("l3_activ"))
        e = conv(a1, "conv7") + conv(a2, "conv9") + conv(a3, "conv10") + b("expand_bias")
        _, _, H, W = e.shape
        d2s = e.reshape(n, f, f, 3, H, W).permute(0, 4, 1, 5, 2, 3).reshape(n, f * H, f * W, 3)
        lin = F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        err = ((lin + d2s - tgt) ** 2).sum()
        p.grad = None
        (err / tgt.numel()).backward()
    return step


def bench(reps, out_path, with_torch=True):
    import torch
    import rusty_sr_amd as r
    params = r.rsr.builtin("imagenet")
    eng = r.Engine(params, device=0, factor=3)
    stream = torch.cuda.current_stream()
    p_d = torch.from_numpy(params).cuda()
    rows = []
    for name, n, h, w in WORKLOADS:
        hr = torch.from_numpy(hr_batch(n, h, w, 1)).cuda()
        grad = torch.empty_like(p_d)
        err = torch.empty(1, dtype=torch.float64, device="cuda")
        med, best = timed(lambda: eng.backprop_dev(hr, p_d, grad=grad, err=err), stream, reps)
        fl = flops_per_call(n, h, w)
        row = {"workload": name, "n": n, "h": h, "w": w, "factor": 3, "lr_pixels": n * (h // 3) * (w // 3),
               "launches_per_call": 16 if h % 3 == 0 else 15 + n, "call_ms": round(med, 4), "call_ms_best": round(best, 4),
               "tflops_call": round(fl / med / 1e9, 2), "peak_share_call": round(fl / med / 1e9 / PEAK_TF, 4)}
        if with_torch:
            torch.backends.cudnn.benchmark = True
            tmed, tbest = timed(torch_step(params, hr), stream, reps)
            row.update({"torch_ms": round(tmed, 4), "torch_ms_best": round(tbest, 4), "speedup_vs_torch": round(tmed / med, 3)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def summarize(d):
    """Per-kernel time of each workload's timed calls, from the rocpd database of the trace (calls begin with the pool kernel)."""
    import collections
    import sqlite3
    files = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not files:
        sys.exit(f"no rocprofv3 database under {d}")
    rows = sqlite3.connect(files[0]).execute("select name, start, end from kernels order by start").fetchall()
    calls, cur = [], None
    for n, s, e in rows:
        if "valid_pool_kernel" in n:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((n, e - s))
    print(f"backprop calls traced: {len(calls)} (8 per workload: 3 warm-up + 5 timed); kernel launches per call: "
          f"{sorted(set(len(k) for k in calls))}")
    for wi, (wname, n, h, w) in enumerate(WORKLOADS):
        sel = calls[wi * 8 + 3:(wi + 1) * 8]
        agg = collections.OrderedDict()
        for call in sel:
            for k, (name, dur) in enumerate(call):
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
                agg.setdefault((k, short), []).append(dur / 1e3)
        tot = sum(sum(v) for v in agg.values()) / len(sel)
        px = n * (h // 3) * (w // 3)
        print(f"\n== {wname} ({n} x {h}x{w} HR): {px} LR pixels; kernel time per call {tot / 1e3:.3f} ms (sum of kernel durations)")
        print(f"{'#':>2s} {'kernel':40s} {'us/call':>10s} {'share':>7s}")
        conv_us = 0.0
        for (k, name), v in agg.items():
            us = sum(v) / len(sel)
            if "grad_conv_kernel" in name or "grad_wgrad_kernel" in name:
                conv_us += us
            print(f"{k:2d} {name[:40]:40s} {us:10.1f} {us / tot:7.3f}")
        fl = flops_per_call(n, h, w)
        print(f"conv kernels (forward, data gradient, weight gradient): {conv_us / 1e3:.3f} ms -> {fl / conv_us / 1e6:.1f} TF/s = "
              f"{fl / conv_us / 1e6 / PEAK_TF:.3f} of the {PEAK_TF} TF f32-MFMA peak; all the call's kernels: {fl / tot / 1e6:.1f} TF/s")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        bench(a.reps, a.out, not a.no_torch)
