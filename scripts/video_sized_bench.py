#!/usr/bin/env python3
"""Times video at any size (include/srhip.h "Video at any size") on 1920x1080 frames, limited-range BT.709, imagenet.rsr,
C420mpeg2 (8-bit) and C420p10.  Fresh processes, the parent commit's built tree (--parent DIR, optional) and this build's interleaved,
`--rounds` rounds; every figure is reported as the median of the rounds' medians with their min and max.
  (1) the fused vertical pass against what it replaces: the 5760x3240 f32 output of a frame -> 3840x2160, lanczos3.  `chain` is
      sr_resize_dev (f32 -> f32) + sr_rgb_to_yuv[16]_dev by hipEvent pairs; `fused` is sr_resize_to_yuv[16]'s launches (sr_last_timing's
      total_ms: taps, horizontal pass, fused vertical pass), with 1 and with 2 row pairs a workgroup ("vyuv").  Both hold the same tap
      and horizontal launches: the difference is resize_v_yuv against resize_v + rgb_to_yuv.  (Kernel times by name: the rocprofv3
      run of scripts/video_sized_rocprof.py.)
  (2) the composed call 1080p -> 2160p in both precisions: total_ms of sr_upscale_yuv[16]_sized against the plain sr_upscale_yuv[16]
      (x3 frames) and against sr_upscale_rgba8_sized at the same sizes.
  (3) the frame stream, 3 slots, 1080p -> 2160p against the plain x3 stream: ms/frame and the bytes downloaded a frame.
  (4) the plain stream and the plain composed call of the parent's tree against this build's (unchanged paths).
    python scripts/video_sized_bench.py [--parent DIR] [--rounds 3] [--reps 10] [--frames 40] [--out profiles/video_sized_bench.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, F, OH, OW = 1080, 1920, 3, 2160, 3840


def med(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def child(root, reps, frames):
    """One process on the package of the tree at `root`: one JSON line a figure."""
    sys.path.insert(0, os.path.join(root, "scripts"))
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import rusty_sr_amd as r
    from border_bench import image, timed
    sized = hasattr(r.Engine, "resize_to_yuv")
    fmts = {"C420mpeg2": r.YuvFormat.named("420", "left", "bt709", "limited"), "C420p10": r.Yuv16Format.named("420", "left", "bt709", "limited", 10)}
    px = image()
    x = px[None, ..., :3].astype(np.float32) / np.float32(255)
    s = torch.cuda.Stream()

    def emit(**row):
        print(json.dumps(row), flush=True)

    for precision in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
        eng.set_profiling(True)

        def total(call, n=reps):
            call()
            call()
            ts = []
            for _ in range(n):
                call()
                ts.append(eng.last_timing()["total_ms"])
            return med(ts)

        for name, fmt in fmts.items():
            deep = name == "C420p10"
            tag = "yuv16" if deep else "yuv"
            frame = getattr(eng, f"rgb_to_{tag}")(x[0], fmt)
            if sized and precision == "f32":   # (1): the launches do not depend on the precision
                with torch.cuda.stream(s):
                    d_net = eng.upscale_f32_dev(torch.from_numpy(x).cuda(), stream=s)
                    d_res = torch.empty((1, OH, OW, 3), dtype=torch.float32, device="cuda")
                    d_out = getattr(eng, f"rgb_to_{tag}_dev")(d_res, fmt, stream=s)
                    chain = lambda: (eng.resize_dev(d_net, (OH, OW), "f32", out=d_res, stream=s),
                                     getattr(eng, f"rgb_to_{tag}_dev")(d_res, fmt, out=d_out, stream=s))
                    for _ in range(4):
                        chain()
                    s.synchronize()
                    t_chain = med(timed(chain, s, 3 * reps))
                    s.synchronize()
                net = d_net.cpu().numpy()
                row = {"fig": "vertical_pass", "format": name, "chain_ms": round(t_chain, 4)}
                for pairs in ("1", "2"):
                    eng.set_experiment("vyuv", pairs)
                    row[f"fused_pairs{pairs}_ms"] = round(total(lambda: getattr(eng, f"resize_to_{tag}")(net, fmt, (OH, OW)), max(3, reps // 2)), 4)
                eng.set_experiment("vyuv", "")
                emit(**row)
                del d_net, d_res, d_out, net
            # (2)
            row = {"fig": "composed", "format": name, "precision": precision,
                   "plain_x3_ms": round(total(lambda: getattr(eng, f"upscale_{tag}")(frame, fmt, H, W)), 4)}
            if sized:
                row["sized_2160p_ms"] = round(total(lambda: getattr(eng, f"upscale_{tag}_sized")(frame, fmt, H, W, (OH, OW))), 4)
            if not deep:
                row["rgba8_sized_2160p_ms"] = round(total(lambda: eng.upscale_rgba8_sized(px[None], (OH, OW))), 4)
            emit(**row)
            # (3), (4)
            if precision == "f32" or not deep:
                for kind in (("plain", None),) + ((("sized", (OH, OW)),) if sized else ()):
                    vs = r.VideoStream(eng, fmt, H, W, slots=3, size=kind[1]) if kind[1] else r.VideoStream(eng, fmt, H, W, slots=3)

                    def run(count):
                        for _ in range(count):
                            if vs.pending == 3:
                                vs.receive(copy=False)
                            vs.submit(frame)
                        while vs.pending:
                            vs.receive(copy=False)
                    run(6)
                    t0 = time.perf_counter()
                    run(frames)
                    emit(fig="stream", format=name, precision=precision, kind=kind[0], ms_per_frame=round(1e3 * (time.perf_counter() - t0) / frames, 4),
                         bytes_down=vs.out_bytes)
                    vs.close()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.frames)
    libs = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("build", ROOT)]
    seen = {}
    for rnd in range(a.rounds):
        for who, lib in libs:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, "--reps", str(a.reps), "--frames", str(a.frames)],
                                 capture_output=True, text=True, timeout=900)
            if res.returncode != 0:
                print(res.stderr[-2000:], file=sys.stderr)
                return res.returncode
            for line in res.stdout.splitlines():
                if line.startswith("{"):
                    row = json.loads(line)
                    key = (who,) + tuple((k, v) for k, v in row.items() if isinstance(v, str))
                    for k, v in row.items():
                        if not isinstance(v, str):
                            seen.setdefault(key, {}).setdefault(k, []).append(v)
    rows = []
    for key, vals in seen.items():
        row = {"lib": key[0], **dict(key[1:]), "rounds": a.rounds}
        for k, v in vals.items():
            row[k] = {"median": med(v), "min": min(v), "max": max(v)} if k != "bytes_down" else v[0]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
