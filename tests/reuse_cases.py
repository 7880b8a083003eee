"""The frames that reach the edge of the row reuse's dependency cone: key frames, changes, formats, sizes and the
sequences whose plans are written down here as literals.  HIP-free; tests/test_reuse_cases_cpu.py holds the premises on the
references alone, tests/test_gpu_reuse_cone.py runs the frames through the sessions.

A change of luma row r is a `checker`: the row becomes white, black, white, ... -- strong enough that every one of the 15 LR rows the
network can carry it to (SR_HALO = 7 on either side) changes in every format below.  It is made as an edit of the RGB picture (one row of
255, 0, 255, ...), converted by the restatement, and taken up in the frame's LUMA plane: the chroma planes keep their samples, so that a
list of dirty rows means the same rows, and the same plan, in every format (a 4:2:0 chroma row that changes dirties four luma rows; it has
cases of its own, `chroma`).  A row that is hit again gets the other phase (black first)."""
import numpy as np

import reuse_ref
import yuv16_ref
import yuv_ref
from conftest import synth_u8

# name -> (subsampling, siting, range, depth), all BT.709
FORMATS = {"420left": ("420", "left", "limited", 8), "444": ("444", "center", "limited", 8), "420p10": ("420", "left", "limited", 10),
           "444p16": ("444", "center", "full", 16), "420p16": ("420", "left", "full", 16)}
SUB = {"420": reuse_ref.SUB_420, "444": reuse_ref.SUB_444}
SMOOTH_SEED, NOISE_SEED = 764, 1


def picture(kind, h, w, seed=None):
    """The key picture as f32 RGB in [0, 1]: "smooth" (tests/conftest.py synth_u8) or "noise" (seeded uniform bytes)."""
    if kind == "smooth":
        px = synth_u8(SMOOTH_SEED if seed is None else seed, 1, h, w)[0]
    else:
        px = np.random.default_rng(NOISE_SEED if seed is None else seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return px.astype(np.float32) / np.float32(255.0)


def to_frame(rgb, name):
    sub, siting, rng, depth = FORMATS[name]
    if depth == 8:
        return yuv_ref.rgb_to_yuv(rgb, sub, siting, "bt709", rng)
    return yuv16_ref.rgb_to_yuv(rgb, sub, siting, "bt709", rng, depth)


def to_rgb(frame, name, h, w):
    sub, siting, rng, depth = FORMATS[name]
    if depth == 8:
        return yuv_ref.yuv_to_rgb(frame, h, w, sub, siting, "bt709", rng)
    return yuv16_ref.yuv_to_rgb(frame, h, w, sub, siting, "bt709", rng, depth)


def key_frame(kind, name, h, w, seed=None):
    return to_frame(picture(kind, h, w, seed), name)


def planes(frame, name, h, w):
    """Views of the frame's Y, Cb, Cr planes."""
    sub, _, _, depth = FORMATS[name]
    return (yuv_ref if depth == 8 else yuv16_ref).split(frame, sub, h, w)


def chroma_limits(name):
    _, _, rng, depth = FORMATS[name]
    return (0, 2 ** depth - 1) if rng == "full" else (16 << (depth - 8), 240 << (depth - 8))


# ---- the changes: ("checker", row), ("chroma", chroma row; negative: from the last), ("tick", row), ("same",) --------------------------
def checker(row):
    return ("checker", row)


def chroma_block(c):
    return ("chroma", c)


def tick(row):
    return ("tick", row)


def checker_luma(name, w, phase):
    """The luma samples of one picture row of 255, 0, 255, ... (phase 1: 0, 255, ...), by the format's own conversion."""
    _, _, rng, depth = FORMATS[name]
    row = np.zeros((1, w, 3), np.float32)
    row[0, phase::2] = 1.0
    if depth == 8:
        return yuv_ref.rgb_to_yuv(row, "444", "center", "bt709", rng)[:w]
    return yuv16_ref.rgb_to_yuv(row, "444", "center", "bt709", rng, depth)[:w]


def apply(frame, change, name, h, w):
    """The frame after the change (a copy)."""
    out = frame.copy()
    y, cb, _ = planes(out, name, h, w)
    kind = change[0]
    if kind == "checker":
        codes = checker_luma(name, w, 0)
        y[change[1]] = checker_luma(name, w, 1) if np.array_equal(y[change[1]], codes) else codes
    elif kind == "chroma":
        assert FORMATS[name][0] == "420"
        lo, hi = chroma_limits(name)
        c = change[1] % cb.shape[0]
        codes = np.where(np.arange(cb.shape[1]) % 2 == 0, hi, lo).astype(cb.dtype)
        if np.array_equal(cb[c], codes):
            codes = (lo + hi - codes).astype(cb.dtype)
        cb[c] = codes
    elif kind == "tick":
        y[change[1], 5] ^= 8
    else:
        assert kind == "same"
    return out


def build(key, changes_per_frame, name, h, w):
    """The key frame and, for every entry, the frame before it with the entry's changes."""
    frames = [key]
    for changes in changes_per_frame:
        cur = frames[-1]
        for ch in changes:
            cur = apply(cur, ch, name, h, w)
        frames.append(cur)
    return frames


# ---- the sequence at h = 160 and h = 161 -------------------------------------------------------------------------------------------------
# (what it covers, the changes against the frame before, the plan at h = 160, the plan at h = 161); "420": 4:2:0 formats only.
# The plans are literals: worked out by hand from the rule in include/srhip.h, not by the code they test.
WHOLE = "whole"
SEQUENCE = (
    ("three bands", [checker(20), checker(80), checker(140)], [(12, 28), (72, 88), (132, 148)], [(12, 28), (72, 88), (132, 148)]),
    ("the frame again", [("same",)], [], []),
    ("four bands, the outer ones at the image edges", [checker(10), checker(56), checker(102), checker(150)],
     [(0, 18), (48, 64), (94, 110), (142, 160)], [(0, 18), (48, 64), (94, 110), (142, 161)]),
    ("five runs merged to four, the smallest gap closed", [checker(9), checker(45), checker(80), checker(116), checker(151)],
     [(0, 18), (38, 88), (108, 124), (144, 160)], [(0, 18), (38, 88), (108, 124), (144, 161)]),
    ("13 clean rows: merged", [checker(40), checker(68)], [(32, 76)], [(32, 76)]),
    ("14 clean rows: two bands", [checker(40), checker(70)], [(32, 48), (62, 78)], [(32, 48), (62, 78)]),
    ("top halo begins at input row 1", [checker(15)], [(8, 24)], [(8, 24)]),
    ("a < SR_HALO: from row 0", [checker(14)], [(0, 22)], [(0, 22)]),
    ("h - b = 8 (at 160): bottom halo ends one row above the last", [checker(144)], [(136, 152)], [(136, 152)]),
    ("h - b < SR_HALO (at 160): to the last row", [checker(145)], [(138, 160)], [(138, 154)]),
    ("rows plus margins reach the frame: whole", [checker(r) for r in (12, 40, 68, 96, 124, 150)], WHOLE, WHOLE),
    ("420: chroma row 30, luma rows 59..62", [chroma_block(30)], [(52, 70)], [(52, 70)]),
    ("420: chroma at the top edge", [chroma_block(0)], [(0, 10)], [(0, 10)]),
    ("420: chroma at the bottom edge", [chroma_block(-1)], [(150, 160)], [(152, 161)]),
)


def sequence(name, h):
    """(labels, changes per frame, plans) of the sequence for a format at h = 160 or 161; WHOLE stands for [(0, h)]."""
    assert h in (160, 161)
    rows = [s for s in SEQUENCE if FORMATS[name][0] == "420" or not s[0].startswith("420:")]
    plans = [[(0, h)] if s[2 + h - 160] == WHOLE else list(s[2 + h - 160]) for s in rows]
    return [s[0] for s in rows], [s[1] for s in rows], plans


def plans_of(frames, name, h, w):
    """The restatement's plan of every frame but the first against the frame before it."""
    sub, _, _, depth = FORMATS[name]
    return [reuse_ref.plan(reuse_ref.frame_flags(a, b, SUB[sub], h, w, 1 if depth == 8 else 2), SUB[sub], h) for a, b in zip(frames, frames[1:])]


def cones(prev, cur, name, h, w):
    """Per band of the frame's plan (none for a whole frame): (band, first LR row, last LR row) of the cone of the RGB-dirty rows inside it."""
    sub, _, _, depth = FORMATS[name]
    flags = reuse_ref.frame_flags(prev, cur, SUB[sub], h, w, 1 if depth == 8 else 2)
    bands = reuse_ref.plan(flags, SUB[sub], h)
    if bands == [(0, h)]:
        return []
    dirty = np.flatnonzero(reuse_ref.dirty_rows(flags, SUB[sub], h))
    out = []
    for a, b in bands:
        d = dirty[(dirty >= a) & (dirty < b)]
        out.append(((a, b), max(0, int(d.min()) - reuse_ref.SR_HALO), min(h - 1, int(d.max()) + reuse_ref.SR_HALO)))
    return out


def witness(upscaled, frames, name, h, w, f):
    """upscaled: the frames' results (samples) from something that is not under test.  Per frame after the first and per band of its
    plan: (frame, band, luma samples that differ from the frame before in the f output rows of the cone's first LR row, the same for
    its last LR row).  Both counts above 0: a pass that computes one row less, on either side, gives other bytes."""
    out = []
    for i in range(1, len(frames)):
        d = planes(upscaled[i - 1], name, f * h, f * w)[0] != planes(upscaled[i], name, f * h, f * w)[0]
        for band, lo, hi in cones(frames[i - 1], frames[i], name, h, w):
            out.append((i, band, int(d[f * lo:f * lo + f].sum()), int(d[f * hi:f * hi + f].sum())))
    return out
