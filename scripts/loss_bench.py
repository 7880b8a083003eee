#!/usr/bin/env python3
"""What the training objective (sr_set_loss: mse, l1, charbonnier) costs at the reference step: batch 4 x 192^2 crops, f = 3, every image
resident.  Prints one JSON line per row (and appends them to --out).

    python scripts/loss_bench.py [--steps 400] [--warmup 40] [--rounds 5] [--out FILE]

  step_abc     ONE process, one session: the three kinds in turn, `--rounds` times over -- set_loss, a warm-up, then the wall time per
               queued step (Trainer.step_crops, one sync at the end) of `--steps` steps.  The spread of a kind over its rounds is the
               run-to-run spread the differences between the kinds are read against.

    python scripts/loss_bench.py --ab OTHER_CHECKOUT [--repeats 3] [--steps 400] [--warmup 40] [--out FILE]

  parent_ab    this build's MSE step against another checkout's step (its parent, which has no sr_set_loss): in turn, each in a fresh
               process (--one KIND --root CHECKOUT), `--repeats` times over.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/loss_bench.py --trace-run
    python scripts/loss_bench.py --summarize DIR [--out FILE]

  loss_kernel  the loss kernel alone under each kind: --trace-run queues a few steps of each kind (the kind is a template argument, so
               every kind is a kernel name of its own), --summarize reads the run's kernel_stats.csv: average time of grad_loss_kernel
               per kind and its share of the step's kernels."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KINDS = ("mse", "l1", "charbonnier")


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


class Session:
    """the reference step on 8 resident images of 480 x 642, origins from a seeded generator"""

    def __init__(self):
        import rusty_sr_amd as r
        from conftest import synth_u8
        params = r.rsr.builtin("imagenet")
        self.eng = r.Engine(params, device=0)
        self.tr = r.Trainer(self.eng, params)
        self.ids = [self.tr.add_image(synth_u8(k, 1, 480, 642)[0]) for k in range(8)]
        assert min(self.ids) >= 0
        self.rng = np.random.default_rng(0)

    def items(self):
        r = self.rng
        return [(self.ids[int(r.integers(0, 8))], int(r.integers(0, 480 - 192)), int(r.integers(0, 642 - 192))) for _ in range(4)]

    def timed(self, steps, warmup):
        """wall ms per queued step, under the objective in force"""
        for _ in range(warmup):
            self.tr.step_crops(self.items(), 192, 192)
        self.tr.sync()
        plan = [self.items() for _ in range(steps)]
        t0 = time.perf_counter()
        for it in plan:
            self.tr.step_crops(it, 192, 192)
        errs = self.tr.sync()
        wall = (time.perf_counter() - t0) / steps * 1e3
        assert len(errs) == steps and all(np.isfinite(errs))
        return wall

    def close(self):
        self.tr.close()
        self.eng.close()


def step_abc(steps, warmup, rounds, out):
    s = Session()
    got = {k: [] for k in KINDS}
    for _ in range(rounds):
        for k in KINDS:
            s.eng.set_loss(k, 1e-3)
            got[k].append(round(s.timed(steps, warmup), 4))
    s.close()
    base = float(np.median(got["mse"]))
    for k in KINDS:
        v = got[k]
        emit({"what": "step_abc", "kind": k, "steps": steps, "warmup": warmup, "wall_ms_per_step": v, "median": round(float(np.median(v)), 4),
              "spread": round(max(v) - min(v), 4), "median_over_mse": round(float(np.median(v)) / base, 4)}, out)


def one(kind, steps, warmup):
    s = Session()
    if hasattr(s.eng, "set_loss"):   # (a parent checkout has none: its step is the squared loss)
        s.eng.set_loss(kind, 1e-3)
    else:
        assert kind == "mse"
    wall = s.timed(steps, warmup)
    s.close()
    return wall


def parent_ab(other, repeats, steps, warmup, out):
    rows = [("parent_mse", other, "mse"), ("mse", ROOT, "mse")]
    got = {label: [] for label, _, _ in rows}
    for _ in range(repeats):
        for label, root, kind in rows:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--one", kind, "--steps", str(steps), "--warmup",
                                  str(warmup)], capture_output=True, text=True, timeout=900)
            assert res.returncode == 0, res.stderr
            got[label].append(json.loads(res.stdout.strip().splitlines()[-1])["wall_ms_per_step"])
    for label, _, _ in rows:
        v = got[label]
        emit({"what": "parent_ab", "row": label, "steps": steps, "warmup": warmup, "wall_ms_per_step": v, "median": round(float(np.median(v)), 4),
              "spread": round(max(v) - min(v), 4)}, out)


def trace_run():
    s = Session()
    for k in KINDS:
        s.eng.set_loss(k, 1e-3)
        for _ in range(20):
            s.tr.step_crops(s.items(), 192, 192)
        s.tr.sync()
    s.close()


def summarize(d, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel_stats.csv under {d}")
    with open(files[0]) as f:
        stats = list(csv.DictReader(f))
    total = sum(float(s["TotalDurationNs"]) for s in stats)
    loss_total = 0.0
    for s in stats:
        m = re.search(r"grad_loss_kernel<([^>]*)>", s["Name"])   # <F, HR_U8, CH, LINEAR, LOSS>
        if not m:
            continue
        loss_total += float(s["TotalDurationNs"])
        emit({"what": "loss_kernel", "kind": KINDS[int(m.group(1).split(",")[-1])], "instance": m.group(1), "calls": int(s["Calls"]),
              "avg_us": round(float(s["AverageNs"]) / 1e3, 3), "min_us": round(float(s.get("MinNs", "nan")) / 1e3, 3),
              "max_us": round(float(s.get("MaxNs", "nan")) / 1e3, 3)}, out)
    emit({"what": "loss_kernel_share", "all_kinds_share_of_traced_kernel_time": round(loss_total / total, 6), "kernels": len(stats)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="", help="another checkout of this project, built: alternate its step with this build's MSE step")
    ap.add_argument("--root", default=ROOT, help="import rusty_sr_amd from this checkout")
    ap.add_argument("--one", default="", choices=["", *KINDS])
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--summarize", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.summarize:
        summarize(a.summarize, a.out)
    elif a.trace_run:
        trace_run()
    elif a.one:
        emit({"what": "step", "kind": a.one, "root": a.root, "wall_ms_per_step": round(one(a.one, a.steps, a.warmup), 4)}, "")
    elif a.ab:
        parent_ab(a.ab, a.repeats, a.steps, a.warmup, a.out)
    else:
        step_abc(a.steps, a.warmup, a.rounds, a.out)


if __name__ == "__main__":
    main()
