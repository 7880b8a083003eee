"""The row-reuse planner of the frame stream (include/srhip.h sr_video_reuse_plan), restated in numpy: which LR rows a frame computes,
from the row flags of its planes.  The C++ (rusty_sr_amd/csrc/sr_plan.cpp) must equal plan() exactly; frame_stats() is what one frame
adds to a session's sr_video_reuse_stats."""
import numpy as np

SR_HALO = 7
MAX_BANDS = 4
SUB_420, SUB_444, SUB_422 = 0, 1, 2


def chroma_rows(sub, h):
    return (h + 1) // 2 if sub == SUB_420 else h


def split_flags(flags, sub, h):
    flags = np.asarray(flags).reshape(-1) != 0
    ch = chroma_rows(sub, h)
    assert flags.size == h + 2 * ch
    return flags[:h], flags[h:h + ch], flags[h + ch:]


def dirty_rows(flags, sub, h):
    """Step 1: the luma rows whose RGB changes."""
    y, cb, cr = split_flags(flags, sub, h)
    dirty = y.copy()
    for c in np.flatnonzero(cb | cr):
        if sub == SUB_420:
            dirty[max(0, 2 * c - 1):min(h - 1, 2 * c + 2) + 1] = True
        else:
            dirty[c] = True
    return dirty


def plan(flags, sub, h):
    """The bands [(y0, y1), ...]: [] = reuse the whole last output, [(0, h)] = the whole frame."""
    dirty = dirty_rows(flags, sub, h)
    # step 2: needed rows
    need = np.zeros(h, bool)
    for d in np.flatnonzero(dirty):
        need[max(0, d - SR_HALO):d + SR_HALO + 1] = True
    # step 3: maximal runs, their edges adjusted
    edges = np.flatnonzero(np.diff(np.concatenate(([0], need.astype(np.int8), [0]))))
    runs = []
    for a, b in zip(edges[0::2], edges[1::2]):
        a, b = int(a) // 2 * 2, min(h, (int(b) + 1) // 2 * 2)
        if a < SR_HALO:
            a = 0
        if h - b < SR_HALO:
            b = h
        runs.append([a, b])
    merged = []
    for a, b in runs:  # top to bottom: fewer than 2 SR_HALO clean rows apart
        if merged and a - merged[-1][1] < 2 * SR_HALO:
            merged[-1][1] = max(merged[-1][1], b)
        else:
            merged.append([a, b])
    while len(merged) > MAX_BANDS:
        gaps = [merged[i + 1][0] - merged[i][1] for i in range(len(merged) - 1)]
        i = gaps.index(min(gaps))  # the first of equal gaps: the pair nearer the top
        merged[i][1] = merged[i + 1][1]
        del merged[i + 1]
    # step 4: the whole frame where the bands and their margins reach it
    if merged and sum(b - a + 2 * SR_HALO for a, b in merged) >= h:
        return [(0, h)]
    return [(a, b) for a, b in merged]


def frame_stats(bands, h):
    """What a frame with this plan adds to the session's counts."""
    whole = bands == [(0, h)]
    return {"frames": 1, "frames_reused": int(not bands), "frames_partial": int(bool(bands) and not whole), "frames_full": int(whole),
            "rows_total": h, "rows_computed": sum(b - a for a, b in bands), "bands": 0 if whole else len(bands)}


def whole_or_nothing(bands, h):
    """The plan of a session the band form does not exist for (members != 1, a bilinear context)."""
    return [(0, h)] if bands else []


def frame_flags(prev, cur, sub, h, w, sample_bytes=1):
    """The compare's flags for two frames given as bytes: Y rows, then Cb rows, then Cr rows."""
    prev, cur = np.asarray(prev).reshape(-1).view(np.uint8), np.asarray(cur).reshape(-1).view(np.uint8)
    ch, cw = chroma_rows(sub, h), (w if sub == SUB_444 else (w + 1) // 2)
    out, at = [], 0
    for rows, cols in ((h, w), (ch, cw), (ch, cw)):
        n = rows * cols * sample_bytes
        out.append((prev[at:at + n].reshape(rows, -1) != cur[at:at + n].reshape(rows, -1)).any(axis=1))
        at += n
    assert at == prev.size == cur.size
    return np.concatenate(out).astype(np.uint32)
