#!/usr/bin/env python3
"""Times the row reuse of the frame stream (include/srhip.h sr_video_set_reuse) on 1920x1080 C420mpeg2 frames, limited-range
BT.709, imagenet.rsr, 3 slots, in both precisions.  Wall clock per frame over blocks of `--frames` frames with the ring kept full; the
sessions with the mode off and on take turns, block by block, `--rounds` times, and the medians of their blocks are compared.
  (a) The compare launch alone (sr_rows_differ_dev over one frame's bytes as rows of the luma width), a hipEvent pair around each launch:
      us, and its share of the 6.3 TB/s HBM copy roof for reading both frames once -- at 1920x1080 and 3840x2160 input.
  (b) Nothing can be reused: every row changes every frame.  Reuse on against reuse off: what the compare, the reference copy and the
      host wait in submit cost.  The project's budget for an opt-in composed path is 1.05 x.
  (c) What it buys, the same clip shape in three variants: static letterbox bars of 138 rows above and below a picture that changes
      every frame; every second frame a repeat of the one before; one changing strip of 64 rows in a static frame.  ms/frame, the share
      of rows the network computed, that share with the halo rows of its bands added (the expectation for the ratio), and the ratio.
    python scripts/video_reuse_bench.py [--frames N] [--rounds N] [--reps N] [--out FILE.jsonl]     (one process; run it again for a repeat)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from border_bench import H, W, ROOF_GBPS, image, median, timed  # noqa: E402

SLOTS = 3
HALO = 7


def clips(frame):
    """name -> the frames a clip cycles through.  `frame` is one 4:2:0 frame; its twin differs from it in one sample of every row of
    every plane."""
    import numpy as np
    ch, cw = (H + 1) // 2, (W + 1) // 2
    twin = frame.copy()
    twin[:H * W].reshape(H, W)[:, 7] ^= 1
    twin[H * W:].reshape(2 * ch, cw)[:, 5] ^= 1

    def rows_from(a, b, y0, y1):   # a with the luma rows [y0, y1) of b and the chroma rows under them (y0, y1 even)
        out = a.copy()
        out[:H * W].reshape(H, W)[y0:y1] = b[:H * W].reshape(H, W)[y0:y1]
        for p in range(2):
            plane, other = out[H * W + p * ch * cw:][:ch * cw].reshape(ch, cw), b[H * W + p * ch * cw:][:ch * cw].reshape(ch, cw)
            plane[y0 // 2:y1 // 2] = other[y0 // 2:y1 // 2]
        return out

    black = np.concatenate([np.full(H * W, 16, np.uint8), np.full(2 * ch * cw, 128, np.uint8)])
    box_a, box_b = rows_from(black, frame, 138, H - 138), rows_from(black, twin, 138, H - 138)
    return {
        "all_rows_change": [frame, twin],
        "letterbox_2x138": [box_a, box_b],
        "every_second_repeated": [frame, frame, twin, twin],
        "strip_64_rows": [frame, rows_from(frame, twin, 500, 564)],
    }


def bench(frames, rounds, reps, out_path):
    import numpy as np
    import torch
    import rusty_sr_amd as r
    fmt = r.YuvFormat.named("420", "left", "bt709", "limited")
    px = image()
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    # (a) the compare launch alone
    s = torch.cuda.Stream()
    eng = r.Engine(r.rsr.builtin("imagenet"), device=0)
    for h, w in ((H, W), (2 * H, 2 * W)):
        fb = r.yuv_frame_bytes(fmt, h, w)
        n_rows = fb // w          # the frame's bytes as rows of the luma width: h + h / 2 of them
        a = torch.randint(0, 256, (fb,), dtype=torch.uint8, device="cuda")
        b = a.clone()
        out = torch.empty((n_rows,), dtype=torch.int32, device="cuda")
        with torch.cuda.stream(s):
            fn = lambda: eng.rows_differ_dev(a, b, n_rows, w, out=out, stream=s)
            for _ in range(8):
                fn()
            s.synchronize()
            ts = timed(fn, s, 4 * reps)
        assert int(out.sum()) == 0
        med, moved = median(ts), 2 * n_rows * w + 4 * n_rows
        emit({"launch": "rows_differ", "size": f"{w}x{h}", "rows": n_rows, "row_bytes": w, "us": round(1e3 * med, 2), "min_us": round(1e3 * min(ts), 2),
              "MB": round(moved / 1e6, 2), "GBps": round(moved / med / 1e6, 1), "frac_of_6.3TBps_copy_roof": round(moved / med / 1e6 / ROOF_GBPS, 4),
              "reps": 4 * reps})
    x = torch.from_numpy(px[None, ..., :3].astype(np.float32) / np.float32(255)).cuda()
    frame = eng.rgb_to_yuv_dev(x, fmt).cpu().numpy()[0]
    eng.close()
    sets = clips(frame)

    # (b), (c) the stream, mode off and on in turns
    for precision in ("f32", "split_f16"):
        eng = r.Engine(r.rsr.builtin("imagenet"), device=0, precision=precision)
        for name, cycle in sets.items():
            streams = {mode: r.VideoStream(eng, fmt, H, W, slots=SLOTS, reuse=mode) for mode in (False, True)}

            def run(vs, count):   # the ring kept full; a received frame is looked at in place, as the CLI writes it from there
                for i in range(count):
                    if vs.pending == SLOTS:
                        vs.receive(copy=False)
                    vs.submit(cycle[i % len(cycle)])
                while vs.pending:
                    vs.receive(copy=False)

            for vs in streams.values():
                run(vs, 16)   # (the engine measures per shape whether a call runs as two bands: settled before anything is timed)
            before = streams[True].reuse_stats()
            per = {False: [], True: []}
            for _ in range(rounds):
                for mode in (False, True):
                    t0 = time.perf_counter()
                    run(streams[mode], frames)
                    per[mode].append(1e3 * (time.perf_counter() - t0) / frames)
            st = {k: v - before[k] for k, v in streams[True].reuse_stats().items()}
            for vs in streams.values():
                vs.close()
            off, on = median(per[False]), median(per[True])
            emit({"clip": name, "precision": precision, "size": f"{W}x{H}", "slots": SLOTS, "frames_per_block": frames, "rounds": rounds,
                  "off_ms_per_frame": round(off, 4), "off_blocks_ms": [round(t, 4) for t in per[False]], "on_ms_per_frame": round(on, 4),
                  "on_blocks_ms": [round(t, 4) for t in per[True]], "on_over_off": round(on / off, 4),
                  "rows_computed_share": round(st["rows_computed"] / st["rows_total"], 4),
                  "rows_with_halos_share": round(min(1.0, (st["rows_computed"] + 2 * HALO * st["bands"]) / st["rows_total"]), 4),
                  "frames_whole": st["frames_full"], "frames_partial": st["frames_partial"], "frames_reused": st["frames_reused"]})
        eng.close()
    if out_path:
        with open(out_path, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    bench(a.frames, a.rounds, a.reps, a.out)


if __name__ == "__main__":
    main()
