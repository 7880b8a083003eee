#!/usr/bin/env python3
"""Where the time of a frame goes on the host with row reuse off and on, 1920x1080 C420mpeg2, 3 slots, every row changing
every frame: wall clock per frame and the mean time the host spends inside submit and inside receive, three rounds of both modes.
    python scripts/video_reuse_where.py f32|split_f16 FRAMES          (GPU_MAX_HW_QUEUES=8 in the environment: the observation of DESIGN.md 4q)
    rocprofv3 --kernel-trace --stats -- python scripts/video_reuse_where.py f32 60 trace      (one short run with the mode on, for a kernel trace)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from border_bench import H, W, image  # noqa: E402
from video_reuse_bench import clips, SLOTS  # noqa: E402


def main():
    import numpy as np
    import torch
    import rusty_sr_amd as r
    precision, frames, trace = sys.argv[1], int(sys.argv[2]), len(sys.argv) > 3
    fmt = r.YuvFormat.named("420", "left", "bt709", "limited")
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
    x = torch.from_numpy(image()[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()
    frame = eng.rgb_to_yuv_dev(x, fmt).cpu().numpy()[0]
    cycle = clips(frame)["all_rows_change"]
    for rnd in range(1 if trace else 3):
        for mode in ((True, ) if trace else (False, True)):
            vs = r.VideoStream(eng, fmt, H, W, slots=SLOTS, reuse=mode)
            t_sub = t_rec = 0.0

            def run(count):
                nonlocal t_sub, t_rec
                for i in range(count):
                    if vs.pending == SLOTS:
                        t = time.perf_counter()
                        vs.receive(copy=False)
                        t_rec += time.perf_counter() - t
                    t = time.perf_counter()
                    vs.submit(cycle[i % 2])
                    t_sub += time.perf_counter() - t
                t = time.perf_counter()
                while vs.pending:
                    vs.receive(copy=False)
                t_rec += time.perf_counter() - t
            run(16)
            t_sub = t_rec = 0.0
            t0 = time.perf_counter()
            run(frames)
            total = time.perf_counter() - t0
            vs.close()
            print(json.dumps({"precision": precision, "hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", ""), "reuse": mode, "round": rnd,
                              "ms_per_frame": round(1e3 * total / frames, 4), "submit_ms": round(1e3 * t_sub / frames, 4),
                              "receive_ms": round(1e3 * t_rec / frames, 4)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
