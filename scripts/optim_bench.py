#!/usr/bin/env python3
"""What the optimiser's options (sr_train_set_optim / sr_train_set_lr: clipping, the parameter average, a rate per step) cost at the
reference step: batch 4 x 192^2 crops, f = 3, every image resident.  Prints one JSON line per row (and appends them to --out).

    python scripts/optim_bench.py --ab OTHER_CHECKOUT [--repeats 3] [--steps 400] [--warmup 40] [--out FILE]

  step_ab      another checkout's step (the parent commit's, which has none of the options), this build's default step and this build's
               step with clipping, the average and a rate set before every step, in turn, each in a fresh process
               (--one KIND --root CHECKOUT), `--repeats` times over: wall time per queued step, one sync at the end.  The spread of a
               row over its repeats is what the differences are read against.

    python scripts/optim_bench.py [--rounds 5] [--steps 400] [--warmup 40] [--out FILE]

  step_modes   ONE process: a default session and one with the options on, in turn, `--rounds` times over.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/optim_bench.py --trace-run
    python scripts/optim_bench.py --summarize DIR [--out FILE]

  optim_kernels  the kernels of sr_optim.hip alone (and grad_adam_kernel beside them): --trace-run queues 40 steps with the options on
               and 40 without, --summarize reads the run's kernel_stats.csv."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KINDS = ("default", "optim")
CLIP, DECAY = 0.05, 0.999   # (a norm the steps of this session cross now and then; the cost does not depend on it)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


class Session:
    """the reference step on 8 resident images of 480 x 642, origins from a seeded generator"""

    def __init__(self, kind):
        import rusty_sr_amd as r
        from conftest import synth_u8
        params = r.rsr.builtin("imagenet")
        self.r = r
        self.eng = r.Engine(params, device=0)
        self.tr = r.Trainer(self.eng, params)
        self.optim = kind == "optim"
        if self.optim:   # (a parent checkout has none of this: its step is the default one)
            self.tr.set_optim(CLIP, DECAY)
            self.sched = r.parse_lr_schedule("cosine:100000", 2e-3, 10)
        self.ids = [self.tr.add_image(synth_u8(k, 1, 480, 642)[0]) for k in range(8)]
        assert min(self.ids) >= 0
        self.rng = np.random.default_rng(0)
        self.t = 0

    def items(self):
        r = self.rng
        return [(self.ids[int(r.integers(0, 8))], int(r.integers(0, 480 - 192)), int(r.integers(0, 642 - 192))) for _ in range(4)]

    def step(self, it):
        self.t += 1
        if self.optim:
            self.tr.set_lr(self.r.lr_at(self.sched, self.t))
        self.tr.step_crops(it, 192, 192)

    def timed(self, steps, warmup):
        """wall ms per queued step"""
        for _ in range(warmup):
            self.step(self.items())
        self.tr.sync()
        plan = [self.items() for _ in range(steps)]
        t0 = time.perf_counter()
        for it in plan:
            self.step(it)
        errs = self.tr.sync()
        wall = (time.perf_counter() - t0) / steps * 1e3
        assert len(errs) == steps and all(np.isfinite(errs))
        return wall

    def close(self):
        self.tr.close()
        self.eng.close()


def step_modes(steps, warmup, rounds, out):
    got = {k: [] for k in KINDS}
    sessions = {k: Session(k) for k in KINDS}
    for _ in range(rounds):
        for k in KINDS:
            got[k].append(round(sessions[k].timed(steps, warmup), 4))
    for s in sessions.values():
        s.close()
    base = float(np.median(got["default"]))
    for k in KINDS:
        v = got[k]
        emit({"what": "step_modes", "kind": k, "steps": steps, "warmup": warmup, "wall_ms_per_step": v, "median": round(float(np.median(v)), 4),
              "spread": round(max(v) - min(v), 4), "median_over_default": round(float(np.median(v)) / base, 4)}, out)


def one(kind, steps, warmup):
    s = Session(kind)
    wall = s.timed(steps, warmup)
    s.close()
    return wall


def step_ab(other, repeats, steps, warmup, out):
    rows = [("parent", other, "default"), ("default", ROOT, "default"), ("clip_ema_lr", ROOT, "optim")]
    got = {label: [] for label, _, _ in rows}
    for _ in range(repeats):
        for label, root, kind in rows:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--one", kind, "--steps", str(steps), "--warmup",
                                  str(warmup)], capture_output=True, text=True, timeout=900)
            assert res.returncode == 0, res.stderr
            got[label].append(json.loads(res.stdout.strip().splitlines()[-1])["wall_ms_per_step"])
    base = float(np.median(got["parent"]))
    for label, _, _ in rows:
        v = got[label]
        emit({"what": "step_ab", "row": label, "steps": steps, "warmup": warmup, "wall_ms_per_step": v, "median": round(float(np.median(v)), 4),
              "spread": round(max(v) - min(v), 4), "median_over_parent": round(float(np.median(v)) / base, 4)}, out)


def trace_run():
    for k in KINDS:
        s = Session(k)
        for _ in range(40):
            s.step(s.items())
        s.tr.sync()
        s.close()


def summarize(d, out):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no kernel_stats.csv under {d}")
    with open(files[0]) as f:
        stats = list(csv.DictReader(f))
    for s in stats:
        if not any(k in s["Name"] for k in ("optim_sumsq_kernel", "optim_norm_kernel", "optim_adam_kernel", "grad_adam_kernel")):
            continue
        emit({"what": "optim_kernels", "kernel": s["Name"][:80], "calls": int(s["Calls"]), "avg_us": round(float(s["AverageNs"]) / 1e3, 3),
              "min_us": round(float(s.get("MinNs", "nan")) / 1e3, 3), "max_us": round(float(s.get("MaxNs", "nan")) / 1e3, 3)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", default="", help="another checkout of this project, built: alternate its step with this build's two")
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
        step_ab(a.ab, a.repeats, a.steps, a.warmup, a.out)
    else:
        step_modes(a.steps, a.warmup, a.rounds, a.out)


if __name__ == "__main__":
    main()
