"""The plan-record case table (tests/golden/plan_cases.json) and the three things done with it: run it against the built library
(tests/golden/make_plan_records.py, tests/test_gpu_plan_records.py), run it through the HIP-free planners (tests/c/plan_check.cpp,
tests/test_plan_cpu.py), and bring both to one form to compare -- per context of a call the lines

    host KIND SIZES [rows=LO:HI]  |  fork 0  |  fork 1 ROWS_A,ROWS_B  |  launch ST FORM TY8 TY4 GRID   (one per launch, in issue order)

The table holds inputs only, in groups: call ("dev" | "band" | "host" | "multi") and, each a list of alternatives of which a group is the
product, ctx [factor, precision], io ("u8": RGB bytes in, RGBA out | "f32"), shape [h, w] and, where they differ from the defaults, n,
halo [top, bottom] (rows of h), set {switch: value}, pipeline, profiling, engines (contexts of a "multi" call, all on one device).  A case
is one member of a group, with its position in the table as "id" and its inputs spelt out as "key", which the records are kept under."""
import gzip
import itertools
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = os.path.join(GOLDEN, "plan_cases.json")
PARENT = os.path.join(GOLDEN, "plan_records_parent.json.gz")
SR_HALO = 7


DEFAULTS = {"n": [1], "halo": [[0, 0]], "set": [{}], "pipeline": [True], "profiling": [False], "engines": [1]}


def load_cases():
    with open(CASES) as f:
        groups = json.load(f)
    cases = []
    for g in groups:
        g = {**DEFAULTS, **g}
        for (factor, precision), io, (h, w), n, halo, sets, pipeline, profiling, engines in itertools.product(
                g["ctx"], g["io"], g["shape"], g["n"], g["halo"], g["set"], g["pipeline"], g["profiling"], g["engines"]):
            c = {"call": g["call"], "factor": factor, "precision": precision, "io": io, "n": n, "h": h, "w": w, "halo": halo, "set": sets,
                 "pipeline": pipeline, "profiling": profiling, "engines": engines}
            cases.append({"id": len(cases), "key": json.dumps(c, sort_keys=True), **c})
    assert len({c["key"] for c in cases}) == len(cases)
    return cases


def load_parent():
    """{"cus": the device's compute units, "records": {case key: [sr_get_experiment("plan") text of each context]}}, recorded once from a
    library built from the commit before the planners moved (gzip of the JSON: the text is 380 KB of launch lines)."""
    with gzip.open(PARENT, "rt") as f:
        return json.load(f)


def save_records(path, blob):
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:  # (no name, no time: the same bytes every time)
        f.write((json.dumps(blob, indent=0) + "\n").encode())


def canonical(text):
    """A plan record's text -> the lines above."""
    from rusty_sr_amd.engine import parse_plan
    rec = parse_plan(text)
    assert not rec["aux"], text
    lines = [f"host {kind} {','.join(map(str, sizes))}" + (f" rows={rows[0]}:{rows[1]}" if rows else "") for kind, sizes, rows in rec["host"]]
    lines += [f"fork 1 {a},{b}" if forked else "fork 0" for forked, a, b in rec["fork"]]
    for l in rec["launches"]:
        lines += [f"launch {l['st']} {l['form']} {l['ty8']} {l['ty4']} {l['grid']}"] * l["count"]
    return lines


# ---- the HIP-free side: tests/c/plan_check.cpp ----
def build_plan_check(tmp_dir, sanitize=True):
    """g++ alone, from sr_plan.cpp alone: that this builds is the check that the planners need no HIP.  sanitize: under ASan and UBSan,
    for the CPU test; a test that runs on the GPU machine builds it plain."""
    exe = os.path.join(str(tmp_dir), "plan_check")
    sanitizers = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *sanitizers, os.path.join(ROOT, "tests", "c", "plan_check.cpp"), os.path.join(ROOT, "rusty_sr_amd", "csrc", "sr_plan.cpp"),
                           "-o", exe])
    return exe


def switch_words(sets):
    """The table's switch values as the fields of sr_plan_env that sr_set_experiment makes of them (sr_api.cpp): what plan_check reads."""
    words = []
    for key, v in sets.items():
        if key == "th":  # one digit for all stages, or five
            words.append("th=" + "".join(d if d in "48" else "0" for d in (v if len(v) == 5 else v[0] * 5)))
        elif key == "pipe":
            words.append(f"pipe={ {'none': 0, 'all': 2}.get(v, 1)}")
        elif key == "rows":  # a leading '=': on alternating streams
            words += [f"rows={v.lstrip('=')}", f"rows_two={int(v.startswith('='))}"]
        elif key == "geo":
            words.append(f"geo={int(v != '0')}")
        elif key == "forkshare":
            words.append(f"forkshare={min(0.9, max(0.1, float(v)))}")
        else:  # numbers as they stand: wino, tail, fork, forkmin, bands
            assert key in ("wino", "tail", "fork", "forkmin", "bands"), key
            words.append(f"{key}={v}")
    return words


def check_line(case, cus):
    """One case as plan_check reads it: key=value words."""
    halo = case["halo"]
    words = [f"id={case['id']}", f"cus={cus}", f"factor={case['factor']}", f"prec={case['precision']}", f"call={case['call']}", f"io={case['io']}",
             f"n={case['n']}", f"h={case['h']}", f"w={case['w']}", f"top={halo[0]}", f"bot={halo[1]}", f"engines={case['engines']}",
             f"pipeline={int(case['pipeline'])}", f"profiling={int(case['profiling'])}"]
    return " ".join(words + switch_words(case["set"]))


def run_plan_check(exe, cases, cus):
    """-> (exit status, {case id: [lines of each context]})"""
    res = subprocess.run([exe], input="".join(check_line(c, cus) + "\n" for c in cases), capture_output=True, text=True, timeout=300)
    out, cur = {}, None
    for line in res.stdout.splitlines():
        if line.startswith("case "):
            cur = out.setdefault(int(line.split()[1]), [])
        elif line.startswith("ctx "):
            cur.append([])
        else:
            cur[-1].append(line)
    return res.returncode, res.stderr, out


# ---- the library side ----
class Runner:
    """Makes each case's call once on device 0, on all-zero pixels, with the fork tuner off; one context per (factor, precision, index),
    kept for the whole table."""

    def __init__(self):
        self._engines = {}

    def _engine(self, factor, precision, k):
        import rusty_sr_amd as r
        from rusty_sr_amd import _lib
        key = (factor, precision, k)
        if key not in self._engines:
            if factor == 3:
                params = r.rsr.builtin("imagenet")
            else:  # (a plan depends on no weight)
                params = (np.random.default_rng(factor).standard_normal(_lib.lib().sr_num_params_factor(factor)) * 0.05).astype(np.float32)
            e = r.Engine(params, device=0, factor=factor, precision=precision)
            e.set_experiment("forktune", "0")
            self._engines[key] = e
        return self._engines[key]

    def cus(self):
        return self._engine(3, "f32", 0).device_info()["compute_units"]

    def run(self, case):
        """-> the plan record's text of each context of the call"""
        import torch
        import rusty_sr_amd as r
        engs = [self._engine(case["factor"], case["precision"], k) for k in range(case["engines"])]
        n, h, w = case["n"], case["h"], case["w"]
        u8 = case["io"] == "u8"
        shape = (n, h, w, 3)
        for e in engs:
            for k, v in case["set"].items():
                e.set_experiment(k, v)
            e.set_pipeline(case["pipeline"])
            e.set_profiling(case["profiling"])
        try:
            e = engs[0]
            if case["call"] == "host":
                x = np.zeros(shape, np.uint8 if u8 else np.float32)
                (e.upscale_rgba8 if u8 else e.upscale_f32)(x)
            elif case["call"] == "multi":
                r.upscale_multi(engs, np.zeros(shape[1:], np.uint8 if u8 else np.float32))
            else:
                x = torch.zeros(shape, dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
                if case["call"] == "band":
                    top, bot = case["halo"]
                    (e.upscale_band_rgba8_dev if u8 else e.upscale_band_f32_dev)(x[0], top, bot)
                else:
                    (e.upscale_rgba8_dev if u8 else e.upscale_f32_dev)(x)
                torch.cuda.synchronize()
            return [e.get_experiment("plan") for e in engs]
        finally:
            for e in engs:
                for k in case["set"]:
                    e.set_experiment(k, "")
                e.set_pipeline(True)
                e.set_profiling(False)

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}
