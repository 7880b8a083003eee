#!/usr/bin/env python3
"""Times the degradation operator (include/srhip.h "Degradation") and appends one JSON line per row to profiles/degrade_bench.jsonl (or --out).
  steps   a training step of batch 4, 192 x 192 HR crops, factor 3, on resident images, three ways: plain (pooled input), paired (LR / HR
          pairs) and degraded (sigma 2, noise 8, quality 60).  A block of --reps steps is queued and the session synced: ms per step.
          One fresh process per (library, round), rounds interleaved; --parent LIB adds the parent commit's library (built from the commit
          before this operator: it has no degraded step, and its three missing symbols are taken out of the binding table before it
          loads), so that the degraded step stands beside the PARENT's paired and plain steps, and this build's plain and paired steps
          and its plain 1080p inference call beside the parent's.  Reported per library and workload: the median over the rounds, and
          the rounds' minimum and maximum.
  launch  sr_degrade_rgba8_dev alone on a 768 x 192 frame (the pixels of a batch of four crops), a hipEvent pair around each call:
          the cheapest setting (all zero, factor 3) and the dearest (sigma 4, noise 8, quality 60, factor 4), interleaved.
    python scripts/degrade_bench.py [--parent libsrhip_parent.so] [--rounds N] [--reps N] [--out FILE.jsonl]
    python scripts/degrade_bench.py --trace-run     (what a `rocprofv3 --kernel-trace --stats` run traces: a few degraded steps and launches)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_SYMBOLS = ("sr_degrade_rgba8", "sr_degrade_rgba8_dev", "sr_train_step_degrade")
DEG = dict(sigma=2.0, noise=8.0, quality=60)


def load(parent):
    from rusty_sr_amd import _lib
    if parent:
        for name in NEW_SYMBOLS:
            _lib.SYMBOLS.pop(name, None)
    import rusty_sr_amd as r
    return r


def images(n=4, h=510, w=510):
    import numpy as np
    from bench import synth_u8
    return [np.ascontiguousarray(synth_u8(20 + i, h, w)) for i in range(n)]


def child(parent, reps):
    """one process: every workload of this library once -> one JSON line"""
    import time
    import numpy as np
    import torch
    r = load(parent)
    from bench import synth_u8
    f, crop, n = 3, 192, 4
    start = r.init_params(f, 1)
    eng = r.Engine(start, device=0, factor=f)
    imgs = images()
    rng = np.random.default_rng(5)
    plan = [[(int(rng.integers(0, len(imgs))), int(rng.integers(0, 510 - crop)) // f * f, int(rng.integers(0, 510 - crop)) // f * f) for _ in range(n)]
            for _ in range(reps)]
    out = {}

    def run(name, make_ids, step):
        tr = r.Trainer(eng, start)
        ids = make_ids(tr)
        for items in plan[:8]:
            step(tr, ids, items)
        tr.sync()
        t0 = time.perf_counter()
        for items in plan:
            step(tr, ids, items)
        tr.sync()
        out[name] = (time.perf_counter() - t0) / len(plan) * 1e3
        tr.close()

    run("plain_step_ms", lambda tr: [tr.add_image(im) for im in imgs],
        lambda tr, ids, items: tr.step_crops([(ids[i], y, x) for i, y, x in items], crop, crop))
    lrs = [np.ascontiguousarray(im.reshape(170, f, 170, f, 3).astype(np.uint16).sum(axis=(1, 3)) // 9).astype(np.uint8) for im in imgs]
    run("paired_step_ms", lambda tr: [tr.add_pair(lr, im) for lr, im in zip(lrs, imgs)],
        lambda tr, ids, items: tr.step_pair_crops([(ids[i], y // f, x // f) for i, y, x in items], crop // f, crop // f))
    if not parent:
        degs = [dict(DEG, seed=k) for k in range(n)]
        run("degraded_step_ms", lambda tr: [tr.add_image(im) for im in imgs],
            lambda tr, ids, items: tr.step_degraded([(ids[i], y, x) for i, y, x in items], degs, crop, crop))
    eng.close()
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0)
    px = torch.from_numpy(synth_u8(2, 1080, 1920)[None]).cuda()
    res = eng.upscale_rgba8_dev(px)
    for _ in range(10):
        eng.upscale_rgba8_dev(px, out=res)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.upscale_rgba8_dev(px, out=res)
    torch.cuda.synchronize()
    out["upscale_1080p_ms"] = (time.perf_counter() - t0) / reps * 1e3
    eng.close()
    print(json.dumps(out), flush=True)


def launch_cases(eng, torch):
    img = torch.from_numpy(images(1, 800, 800)[0]).cuda()
    cheap = lambda: eng.degrade_dev(img, 3, window=(8, 8, 768, 192), out=out3)
    dear = lambda: eng.degrade_dev(img, 4, sigma=4.0, noise=8.0, quality=60, window=(8, 8, 768, 192), out=out4)
    out3 = torch.empty((256, 64, 3), dtype=torch.uint8, device="cuda")
    out4 = torch.empty((192, 48, 3), dtype=torch.uint8, device="cuda")
    return [("all zero, factor 3", cheap), ("sigma 4, noise 8, quality 60, factor 4", dear)]


def bench_launch(reps, rounds):
    import torch
    r = load(False)
    eng = r.Engine(graph="bilinear")
    cases = launch_cases(eng, torch)
    s = torch.cuda.current_stream()
    for _, fn in cases:
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in cases]
    for _ in range(rounds):
        for k, (_, fn) in enumerate(cases):
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(s)
                fn()
                b.record(s)
                b.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3)
    eng.close()
    rows = []
    for (name, _), t in zip(cases, times):
        t.sort()
        rows.append({"bench": "launch", "setting": name, "frame": "768x192", "us": round(t[len(t) // 2], 2), "min_us": round(t[0], 2),
                     "p10_us": round(t[len(t) // 10], 2), "p90_us": round(t[len(t) * 9 // 10], 2), "calls": len(t)})
    return rows


def trace_run():
    import torch
    r = load(False)
    eng = r.Engine(r.init_params(3, 1), device=0, factor=3)
    tr = r.Trainer(eng, r.init_params(3, 1))
    ids = [tr.add_image(im) for im in images()]
    for _ in range(6):
        tr.step_degraded([(i, 30, 60) for i in ids], [dict(DEG, seed=k) for k in range(4)], 192, 192)
    tr.sync()
    tr.close()
    for _, fn in launch_cases(eng, torch):
        for _ in range(6):
            fn()
    torch.cuda.synchronize()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="the parent commit's libsrhip.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_bench.jsonl"))
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--child", choices=["this", "parent"])
    a = ap.parse_args()
    if a.trace_run:
        return trace_run()
    if a.child:
        return child(a.child == "parent", a.reps)
    libs = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("this", None)]
    got = {name: [] for name, _ in libs}
    for _ in range(a.rounds):  # interleaved: every round runs each library once, in a process of its own
        for name, path in libs:
            env = dict(os.environ)
            if path:
                env["SRHIP_LIB"] = path
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)], env=env, capture_output=True,
                                 text=True, timeout=600)
            if res.returncode != 0:
                sys.exit(f"{name}: exit {res.returncode}\n{res.stderr[-2000:]}")
            got[name].append(json.loads(res.stdout.strip().splitlines()[-1]))
    rows = []
    for name, _ in libs:
        for key in got[name][0]:
            v = sorted(g[key] for g in got[name])
            rows.append({"bench": "steps", "library": name, "workload": key, "ms": round(v[len(v) // 2], 4), "rounds_min_ms": round(v[0], 4),
                         "rounds_max_ms": round(v[-1], 4), "rounds": len(v), "reps": a.reps})
    med = {(r_["library"], r_["workload"]): r_["ms"] for r_ in rows}
    base = "parent" if a.parent else "this"
    rows.append({"bench": "steps", "summary": f"degraded step / {base}'s paired step", "ratio": round(med[("this", "degraded_step_ms")] / med[(base, "paired_step_ms")], 4),
                 f"degraded / {base}'s plain step": round(med[("this", "degraded_step_ms")] / med[(base, "plain_step_ms")], 4)})
    rows += bench_launch(a.reps, a.rounds)
    with open(a.out, "a") as f:
        for row in rows:
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
