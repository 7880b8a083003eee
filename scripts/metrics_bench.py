#!/usr/bin/env python3
"""Times the Y-PSNR / SSIM scoring pass (include/srhip.h "Metrics") at factor 3 on u8 RGBA HR images of 1920x1080 and 3840x2160:
  * plain_ms   -- sr_validation_error_rgba8_dev (pool + network + loss), a hipEvent pair around it on its stream;
  * scored_ms  -- sr_pool_validation_metrics_rgba8_dev, the same call with the scores, the same way; score_ms = scored_ms - plain_ms;
  * net_ms     -- the network alone on an LR image of the same size (sr_upscale_f32_dev), which the scoring pass must stay below;
  * image_ms   -- sr_image_metrics_rgba8_dev on two u8 images of the HR size (no network);
  * bytes / f64 FLOP of the scoring pass from its shapes (the tile plan of sr_metrics.hip), and the rates they give over score_ms.
    python scripts/metrics_bench.py [--reps N] [--out FILE.jsonl] [--size WxH] [--precision f32|split_f16]
    python scripts/metrics_bench.py --ab PARENT_LIB.so [--rounds N]   the plain host call sr_validation_error_rgba8 at 1920x1080 on this
                                                           build against another build of the library, interleaved, one fresh process per
                                                           (library, round): the difference beside the spread of each library's own rounds
    python scripts/metrics_bench.py --bundled [--out FILE.txt]   Y-PSNR / SSIM of the three bundled parameter sets, plain and ensemble of 8,
                                                           on the pooled goldens under tests/golden/
    python scripts/metrics_bench.py --summarize DIR       the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of this script"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from validation_bench import SIZES, hr_image, timed  # noqa: E402

T, CH_B = 32, 4  # the kernel's tile (SR_METRICS_TILE); RGBA8 HR images


def work(w, h, shave=3, a_bytes=12):
    """Bytes the scoring pass reads from HBM and f64 FLOP it needs (an FMA = 2), from the shapes: tiles of T x T region pixels, each
    loading (T + 10)^2 pixels of both operands (fewer at the region's edge), a row filter over (T + 10) x T positions and a column filter
    over T x T positions, 5 quantities x 11 taps each, 3 products per row-filter tap and 14 operations per map value."""
    rh, rw = h - 2 * shave, w - 2 * shave
    nbytes = flop = 0
    for ry in range(0, rh, T):
        rows, wr = min(T + 10, rh - ry), max(0, min(T, rh - 10 - ry))
        for rx in range(0, rw, T):
            cols, wc = min(T + 10, rw - rx), max(0, min(T, rw - 10 - rx))
            nbytes += rows * cols * (a_bytes + CH_B)
            if wr and wc:
                flop += (wr + 10) * wc * 11 * (5 * 2 + 3) + wr * wc * (55 * 2 + 14)
    return nbytes, flop


def bench(reps, out_path, sizes, precisions):
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
            d_a = torch.from_numpy(hr_image(w, h, w + 1)).cuda()
            res = torch.empty(1, dtype=torch.float64, device="cuda")
            res16 = torch.empty(16, dtype=torch.uint8, device="cuda")
            lr = torch.rand((1, h // 3, w // 3, 3), device="cuda")
            out = torch.empty((1, h, w, 3), device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                # interleaved: plain, scored, plain, scored -- the medians of each
                plain, scored = [], []
                for _ in range(3):
                    plain.append(timed(lambda: eng.validation_error_dev(d_hr, out=res, stream=s), s, reps)[0])
                    scored.append(timed(lambda: eng.validation_metrics_dev(d_hr, err=res, out=res16, stream=s), s, reps)[0])
                net_ms, _ = timed(lambda: eng.upscale_f32_dev(lr, out=out, stream=s), s, reps)
                image_ms, _ = timed(lambda: eng.image_metrics_dev(d_a, d_hr, out=res16, stream=s), s, reps)
            plain_ms, scored_ms = sorted(plain)[1], sorted(scored)[1]
            score_ms = scored_ms - plain_ms
            nbytes, flop = work(w, h)
            m = r.metrics_from_bytes(res16.cpu().numpy(), h, w, 3)
            row = {"precision": precision, "hr": f"{w}x{h}", "plain_ms": round(plain_ms, 4), "plain_rounds_ms": [round(v, 4) for v in plain],
                   "scored_ms": round(scored_ms, 4), "scored_rounds_ms": [round(v, 4) for v in scored], "score_ms": round(score_ms, 4),
                   "score_share_of_call": round(score_ms / scored_ms, 4), "net_ms": round(net_ms, 4), "score_over_net": round(score_ms / net_ms, 4),
                   "image_metrics_ms": round(image_ms, 4), "score_mbytes": round(nbytes / 1e6, 1), "score_f64_gflop": round(flop / 1e9, 3),
                   "score_tbps": round(nbytes / score_ms / 1e9, 3), "score_f64_tflops": round(flop / score_ms / 1e9, 3),
                   "image_metrics_f64_tflops": round(flop / image_ms / 1e9, 3), "y_psnr_of_two_random_images": m["y_psnr"], "reps": reps}
            print(json.dumps(row), flush=True)
            rows.append(row)
        eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


# The plain host call through ctypes alone: a parent build of the library lacks the symbols the package's binding table resolves.
AB_CHILD = r'''
import ctypes as C, json, sys, time
import numpy as np
import torch  # (its HIP runtime first, as rusty_sr_amd._lib does)
sys.path.insert(0, %r); sys.path.insert(0, %r)
from validation_bench import hr_image
from rusty_sr_amd import rsr
L = C.CDLL(sys.argv[1])
reps = int(sys.argv[2])
p = np.ascontiguousarray(rsr.builtin("imagenet"), dtype=np.float32)
ctx = C.c_void_p()
assert L.sr_create(C.byref(ctx), p.ctypes.data_as(C.c_void_p), C.c_size_t(p.size), 3, 0) == 0
hr = hr_image(1920, 1080, 1920)
err, n = C.c_double(), C.c_size_t()
def call():
    assert L.sr_validation_error_rgba8(ctx, hr.ctypes.data_as(C.c_void_p), 4, 1080, 1920, 0, C.byref(err), C.byref(n)) == 0
for _ in range(5):
    call()
walls = []
for _ in range(reps):
    t = time.perf_counter(); call(); walls.append((time.perf_counter() - t) * 1e3)
L.sr_set_profiling(ctx, 1)
devs = []
tot = C.c_double()
for _ in range(reps):
    call(); L.sr_last_timing(ctx, C.byref(tot), None, None, None); devs.append(tot.value)
L.sr_destroy(ctx)
print(json.dumps({"wall_ms": sorted(walls)[reps // 2], "device_ms": sorted(devs)[reps // 2], "err_sum": err.value.hex()}))
''' % (ROOT, os.path.join(ROOT, "scripts"))


def ab(parent_lib, rounds, reps, out_path):
    libs = {"parent": os.path.abspath(parent_lib), "this": os.path.join(ROOT, "rusty_sr_amd", "libsrhip.so")}
    res = {k: [] for k in libs}
    for _ in range(rounds):
        for name, path in libs.items():
            r = subprocess.run([sys.executable, "-c", AB_CHILD, path, str(reps)], capture_output=True, text=True, timeout=300)
            if r.returncode != 0:  # a child that failed may have faulted the GPU: start nothing more on it
                print(name, "FAILED", r.returncode, r.stderr[-500:])
                sys.exit(1)
            res[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    row = {"call": "sr_validation_error_rgba8 1920x1080 f32, host call", "rounds": rounds, "reps": reps}
    for name, v in res.items():
        for key in ("wall_ms", "device_ms"):
            vals = sorted(d[key] for d in v)
            row[f"{name}_{key}"] = round(vals[len(vals) // 2], 4)
            row[f"{name}_{key}_rounds"] = [round(d[key], 4) for d in v]
        row[f"{name}_err_sum"] = v[0]["err_sum"]
    row["same_bits"] = row["parent_err_sum"] == row["this_err_sum"]
    for key in ("wall_ms", "device_ms"):
        spread = max(row[f"parent_{key}_rounds"]) - min(row[f"parent_{key}_rounds"])
        row[f"{key}_difference"] = round(row[f"this_{key}"] - row[f"parent_{key}"], 4)
        row[f"{key}_parent_spread"] = round(spread, 4)
    print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(json.dumps(row) + "\n")


def bundled(out_path):
    import numpy as np
    from PIL import Image
    import rusty_sr_amd as r
    golden = os.path.join(ROOT, "tests", "golden")
    names = ("cartoon_rsa.png", "butterfly_rs.png", "logo_nn.png")
    imgs = [np.array(Image.open(os.path.join(golden, n)).convert("RGBA")) for n in names]
    lines = ["Y-PSNR / SSIM (benchmark protocol: 8-bit BT.601 luma of the quantised output, shave 3, per-image means) and the reference's pooled",
             "RGB PSNR of the bundled parameter sets on tests/golden/ " + ", ".join(f"{n} ({i.shape[1]}x{i.shape[0]})" for n, i in zip(names, imgs)),
             "pooled by 3 (rusty_sr validate --metrics [--ensemble 8]); exact f32", "",
             f"{'parameters':16s} {'ensemble':>8s} {'PSNR':>9s} {'Y-PSNR':>9s} {'SSIM':>9s}"]
    for name in ("imagenet", "imagenetlinear", "anime"):
        eng = r.Engine(r.rsr.builtin(name), device=0)
        for members, label in ((None, "-"), (r._lib.SR_ENSEMBLE_ALL, "8")):
            m = r.validation_metrics([eng], imgs, members=members)
            lines.append(f"{name:16s} {label:>8s} {m['psnr']:9.4f} {m['y_psnr']:9.4f} {m['ssim']:9.6f}")
        eng.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)


def summarize(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel_stats.csv under {d}")
    with open(files[0]) as f:
        stats = list(csv.DictReader(f))
    total = sum(float(s["TotalDurationNs"]) for s in stats)
    print(f"{'kernel':80s} {'calls':>6s} {'avg us':>9s} {'share':>7s}")
    for s in sorted(stats, key=lambda s: -float(s["TotalDurationNs"])):
        print(f"{s['Name'][:80]:80s} {int(s['Calls']):6d} {float(s['AverageNs']) / 1e3:9.2f} {float(s['TotalDurationNs']) / total:7.2%}")
    for w, h in SIZES:
        nbytes, flop = work(w, h)
        print(f"{w}x{h}: the scoring pass reads {nbytes / 1e6:.1f} MB and needs {flop / 1e9:.3f} f64 GFLOP")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="", help="another build of libsrhip.so to compare the plain validation call with")
    ap.add_argument("--bundled", action="store_true")
    ap.add_argument("--summarize", default="")
    ap.add_argument("--size", default="", help="WxH: this HR size only")
    ap.add_argument("--precision", default="f32", help="f32 | split_f16 | both")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    elif a.ab:
        ab(a.ab, a.rounds, a.reps, a.out)
    elif a.bundled:
        bundled(a.out)
    else:
        sizes = [tuple(int(v) for v in a.size.split("x"))] if a.size else SIZES
        bench(a.reps, a.out, sizes, ("f32", "split_f16") if a.precision == "both" else (a.precision,))


if __name__ == "__main__":
    main()
