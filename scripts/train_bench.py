#!/usr/bin/env python3
"""The training session at the reference step (4 x 192^2 crops, f = 3, all images resident) and `rusty_sr train` with its image store
against the same folder forced transient (--store 0).  Prints one JSON line per measurement (and appends them to --out).

    python scripts/train_bench.py [--steps 1000] [--warmup 100] [--no-cli] [--out FILE]

  session      wall time per step of Trainer.step_crops (queued, one sync at the end) -- what the host sustains
  device       HIP events around the same number of sr_backprop_rgba8_dev + sr_adam_step_dev calls on a pre-cut batch: the device
               time of a step without its crop gather (the crop kernel's own time: run this under rocprofv3 --kernel-trace --stats)
  cli          steps/s of `rusty_sr train --timing` on a generated folder, with the store and with --store 0

    python scripts/train_bench.py --ab OTHER_CHECKOUT [--repeats 3] [--steps 1000] [--warmup 100] [--out FILE]

  The paired step against the pooled step, and this build against another (its parent): in turn, each in a fresh process and
  `--repeats` times over, the other checkout's pooled session step, this build's pooled step and this build's paired step
  (sr_train_step_pairs on resident LR / HR pairs, LR crops of 64 x 64) -- same images, same origins.  The spread of each row over its
  repeats is the run-to-run spread the differences are read against.  (--one MODE: a single such measurement, of the package under
  --root.)  With --augment the other checkout's paired step and this build's two augmented steps (every item a member uniform over
  0..7, from a generator of its own: the origins stay those of the other rows) join the rows.  The augmented gather's share of a step:
  run `--one pooled_aug` (or paired_aug) under rocprofv3 --kernel-trace --stats; `--members 4,5,6,7` draws from one class of members."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def session_bench(steps, warmup, out):
    import torch
    import rusty_sr_amd as r
    from conftest import synth_u8
    params = r.rsr.builtin("imagenet")
    eng = r.Engine(params, device=0)
    rng = np.random.default_rng(0)
    imgs = [synth_u8(k, 1, 480, 640)[0] for k in range(8)]
    tr = r.Trainer(eng, params)
    ids = [tr.add_image(im) for im in imgs]
    assert min(ids) >= 0

    def items():
        return [(ids[int(rng.integers(0, len(ids)))], int(rng.integers(0, 480 - 192)), int(rng.integers(0, 640 - 192))) for _ in range(4)]
    for _ in range(warmup):
        tr.step_crops(items(), 192, 192)
    tr.sync()
    plan = [items() for _ in range(steps)]
    t0 = time.perf_counter()
    for it in plan:
        tr.step_crops(it, 192, 192)
    errs = tr.sync()
    wall = (time.perf_counter() - t0) / steps * 1e3
    assert len(errs) == steps and all(np.isfinite(errs))
    tr.close()
    # backprop + Adam alone, on one batch already on the device, on torch's stream
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(params.copy()).to(dev)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    err = torch.empty(1, dtype=torch.float64, device=dev)
    hr = torch.from_numpy(np.stack([im[:192, :192] for im in imgs[:4]])).to(dev).contiguous()
    for t in range(1, warmup + 1):
        eng.backprop_dev(hr, p, False, None, 1e-6, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for t in range(warmup + 1, warmup + steps + 1):
        eng.backprop_dev(hr, p, False, None, 1e-6, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
    e1.record()
    torch.cuda.synchronize()
    device_ms = e0.elapsed_time(e1) / steps
    eng.close()
    emit({"what": "session", "steps": steps, "wall_ms_per_step": round(wall, 4), "steps_per_s": round(1e3 / wall, 1),
          "backprop_adam_device_ms_per_step": round(device_ms, 4), "wall_over_device": round(wall / device_ms, 4)}, out)


def one_step_bench(mode, steps, warmup, members=tuple(range(8))):
    """wall ms per queued session step at the reference step: mode "pooled" (step_crops on HR images) or "paired" (step_pair_crops);
    "pooled_aug" / "paired_aug": the same with a random member per item, uniform over `members`"""
    import rusty_sr_amd as r
    from conftest import synth_u8
    params = r.rsr.builtin("imagenet")
    eng = r.Engine(params, device=0)
    rng = np.random.default_rng(0)
    imgs = [synth_u8(k, 1, 480, 642)[0] for k in range(8)]
    tr = r.Trainer(eng, params)
    aug = mode.endswith("_aug")
    krng = np.random.default_rng(1)
    member = (lambda: (int(members[int(krng.integers(0, len(members)))]),)) if aug else (lambda: ())
    if mode.startswith("paired"):
        lrs = [np.ascontiguousarray(im.reshape(160, 3, 214, 3, 3)[:, 1, :, 1]) for im in imgs]  # (any LR image will do for the timing)
        ids = [tr.add_pair(lr, im) for lr, im in zip(lrs, imgs)]
        step = lambda it: tr.step_pair_crops([i + member() for i in it], 64, 64)
    else:
        ids = [tr.add_image(im) for im in imgs]
        step = lambda it: tr.step_crops([(i, 3 * y, 3 * x) + member() for i, y, x in it], 192, 192)
    assert min(ids) >= 0

    def items():  # origins in LR pixels
        return [(ids[int(rng.integers(0, len(ids)))], int(rng.integers(0, 160 - 64)), int(rng.integers(0, 214 - 64))) for _ in range(4)]
    for _ in range(warmup):
        step(items())
    tr.sync()
    plan = [items() for _ in range(steps)]
    t0 = time.perf_counter()
    for it in plan:
        step(it)
    errs = tr.sync()
    wall = (time.perf_counter() - t0) / steps * 1e3
    assert len(errs) == steps and all(np.isfinite(errs))
    tr.close()
    eng.close()
    return wall


def ab_bench(other, repeats, steps, warmup, out, augment=False):
    rows = [("parent_pooled", other, "pooled"), ("pooled", ROOT, "pooled"), ("paired", ROOT, "paired")]
    if augment:
        rows = [rows[0], ("parent_paired", other, "paired"), *rows[1:], ("pooled_aug", ROOT, "pooled_aug"), ("paired_aug", ROOT, "paired_aug")]
    got = {label: [] for label, _, _ in rows}
    for _ in range(repeats):
        for label, root, mode in rows:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--one", mode, "--steps", str(steps), "--warmup",
                                  str(warmup)], capture_output=True, text=True, timeout=900)
            assert res.returncode == 0, res.stderr
            got[label].append(json.loads(res.stdout.strip().splitlines()[-1])["wall_ms_per_step"])
    for label, _, _ in rows:
        v = got[label]
        emit({"what": "augment_ab" if augment else "pairs_ab", "row": label, "steps": steps, "warmup": warmup, "wall_ms_per_step": v, "median": round(float(np.median(v)), 4),
              "spread": round(max(v) - min(v), 4)}, out)


def cli_bench(steps, out):
    from PIL import Image
    from conftest import synth_u8
    from rusty_sr_amd.build import build_host
    cli = build_host()
    with tempfile.TemporaryDirectory() as d:
        folder = os.path.join(d, "train")
        os.mkdir(folder)
        for k in range(16):  # 16 images of 1080 x 1440: decoding one costs what a large training image costs
            Image.fromarray(synth_u8(100 + k, 1, 1080, 1440)[0]).save(os.path.join(folder, f"{k:02d}.png"))
        for label, extra in (("resident", []), ("transient", ["--store", "0"])):
            res = subprocess.run([cli, "train", os.path.join(d, "o.rsr"), folder, "--steps", str(steps), "--seed", "1", "--timing", *extra],
                                 capture_output=True, text=True, timeout=1200)
            assert res.returncode == 0, res.stderr
            m = re.search(r"([\d.]+) steps/s", res.stderr)
            emit({"what": "cli", "store": label, "steps": steps, "steps_per_s": float(m.group(1)), "timing": res.stderr.strip()}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--cli-steps", type=int, default=400)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="", help="another checkout of this project, built: alternate its pooled step with this build's steps")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--root", default=ROOT, help="import rusty_sr_amd from this checkout")
    ap.add_argument("--one", default="", choices=["", "pooled", "paired", "pooled_aug", "paired_aug"])
    ap.add_argument("--augment", action="store_true", help="with --ab: add the parent's paired row and this build's augmented rows")
    ap.add_argument("--members", default="0,1,2,3,4,5,6,7", help="with --one *_aug: the members an item's member is drawn from")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.one:
        members = tuple(int(k) for k in a.members.split(","))
        emit({"what": "step", "mode": a.one, "root": a.root, "members": list(members) if a.one.endswith("_aug") else [0],
              "wall_ms_per_step": round(one_step_bench(a.one, a.steps, a.warmup, members), 4)}, "")
        return
    if a.ab:
        ab_bench(a.ab, a.repeats, a.steps, a.warmup, a.out, a.augment)
        return
    session_bench(a.steps, a.warmup, a.out)
    if not a.no_cli:
        cli_bench(a.cli_steps, a.out)


if __name__ == "__main__":
    main()
