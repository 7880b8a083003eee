#!/usr/bin/env python3
"""Within-probe A/B of libsrhip builds (scripts/build_variant.sh): interleaved rounds, one fresh process per
(library, round), per-stage medians of HIP-event times on the device-resident 1080p (or HxW) workload.
    python scripts/ab_libs.py [--prec split_f16] [--rounds 3] [--hw 1080x1920] [--entry dev] lib1.so lib2.so ...
--prec, --hw and --entry take comma-separated lists: every combination is measured in each process.  --entry host times the
host-pointer call (upload, kernels, download).  A library given twice is measured as two entries: what separates them is the
run's own spread."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, time, numpy as np, torch
sys.path.insert(0, %r)
import rusty_sr_amd as r
from bench import synth_u8
precs, shapes, entries, reps = sys.argv[1].split(","), sys.argv[2].split(","), sys.argv[3].split(","), int(sys.argv[4])
for prec in precs:
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=prec)
    for hw in shapes:
        H, W = map(int, hw.split("x"))
        host = synth_u8(2, H, W)[None]
        for entry in entries:
            if entry == "host":
                call = lambda: eng.upscale_rgba8(host)
            else:
                px = torch.from_numpy(host).cuda()
                out = eng.upscale_rgba8_dev(px)
                call = lambda: eng.upscale_rgba8_dev(px, out=out)
            for _ in range(10):
                call()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) / reps * 1e3
            eng.set_profiling(True)
            acc = []
            for _ in range(reps):
                call(); torch.cuda.synchronize(); acc.append(eng.last_timing()["stage_ms"])
            eng.set_profiling(False)
            print(json.dumps({"key": [prec, hw, entry], "stages": np.median(np.array(acc), axis=0).tolist(), "wall": wall}), flush=True)
''' % ROOT

ap = argparse.ArgumentParser()
ap.add_argument("--prec", default="split_f16")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--hw", default="1080x1920")
ap.add_argument("--entry", default="dev", help="dev: sr_upscale_rgba8_dev on device buffers; host: sr_upscale_rgba8 on host memory")
ap.add_argument("--per-round", action="store_true", help="also print stage 2's and the wall time of every round")
ap.add_argument("libs", nargs="+")
a = ap.parse_args()
res = {}
for rnd in range(a.rounds):
    for k, lib in enumerate(a.libs):
        path, *envs = lib.split("@")  # lib.so@SRHIP_TAIL=0@SRHIP_BW=8 ...
        env = dict(os.environ, SRHIP_LIB=os.path.abspath(path), **dict(e.split("=", 1) for e in envs))
        r = subprocess.run([sys.executable, "-c", CHILD, a.prec, a.hw, a.entry, str(a.reps)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:  # a child that failed may have faulted the GPU: start nothing more on it
            print(lib, "FAILED", r.returncode, r.stderr[-500:])
            sys.exit(1)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                res.setdefault(tuple(d["key"]), {}).setdefault((k, lib), []).append(d["stages"] + [sum(d["stages"]), d["wall"]])
for (prec, hw, entry), libs in res.items():
    for (_, lib), v in libs.items():
        m = np.median(np.array(v), axis=0)
        mn = np.min(np.array(v), axis=0)
        print(f"{prec} {hw} {entry} {os.path.basename(lib):40s} stages {' '.join(f'{x:7.4f}' for x in m[:5])}  sum {m[5]:.4f}  wall {m[6]:.4f}  (min sum {mn[5]:.4f})", flush=True)
        if a.per_round:  # what each round gave: the spread between a library's own rounds is the A/B's noise floor
            print(f"    rounds: stage 2 {' '.join(f'{r[2]:.4f}' for r in v)} | wall {' '.join(f'{r[6]:.4f}' for r in v)}", flush=True)
