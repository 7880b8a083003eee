"""The grid cells of the pixel operators around the network -- border pad and crop (sr_border.hip), alpha bleed and merge (sr_alpha.hip),
the resampler's two passes (sr_resize.hip) -- and the smallest shapes that reach them.  All of those kernels fold the batch, the row
groups and the column blocks into blockIdx.x, and pad, crop and merge cut their 16-byte groups on the destination ADDRESS, so that the
last column block of a row may hold only the one to three dwords a misaligned row pushes right.  Each case below names the cell it is
meant for -- the `op` line the library writes into the plan record (Engine.last_plan()["ops"]) for that launch -- and
tests/test_gpu_operator_grids.py asserts that cell on the record after every call: a case whose record says otherwise fails.  The
constants the shapes are derived from (1024 dwords of a row per workgroup of a pad or crop, one row of a pad and four of a crop per
block row; 256 pixels x 4 LR rows per workgroup of a merge; 32 x 32 tiles of a bleed; 256 output columns per workgroup of either resize
pass, 4 rows per group, 40960 bytes of LDS for the staged rows) are NOT restated as arithmetic here: the expected cells are written out.

No GPU and no HIP here: tests/test_operator_grids_cpu.py checks on the restatements alone (border_ref, alpha_ref, resize_ref) that the
cases build, that the images of a batch differ, and that every resize case is well enough conditioned for the bar it is held to."""
import numpy as np

import alpha_ref
import pixel_classes as pc
import resize_ref

OFFSETS = (0, 4, 8, 12)   # byte offsets of a buffer within a 16-byte aligned allocation
TOL = 1e-5                # the f32 bar of tests/test_gpu_resize.py (and of tests/test_gpu_parity.py for the parameter-free graphs)
GATE = 0.25               # a resize case stays only if the f32-rounded restatement is within this share of its bar of the f64 one


def cell_mismatch(op, want):
    """The fields of a recorded op that are not what the case expects ({} = the intended cell ran)."""
    return {k: (op.get(k), v) for k, v in want.items() if op.get(k) != v}


# ---- pad and crop: pure dword moves, any bit pattern --------------------------------------------------------------------------------
def dword_image(seed, px, n, h, w):
    """(n, h, w, 4) u8 or (n, h, w, 3) f32 of random bits, NaNs included: the kernels only move dwords."""
    rng = np.random.default_rng(seed)
    if px == "u8":
        return rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    return rng.integers(0, 1 << 32, (n, h, w, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)


# (px, n, h, w, pad, what it is for); every mode, output at every offset.  A padded row of R dwords: the second block of a row holds
# dwords only where (start of the row in dwords) mod 4 + R > 1024.
PAD_CASES = [
    ("u8", 3, 3, 1006, 8, "1022 dwords: the second block holds nothing but one spilled dword, on rows that start 3 dwords off"),
    ("u8", 3, 3, 1007, 8, "1023 dwords, odd: the start of a row rotates through all four residues; spills of 1 and 2 dwords"),
    ("u8", 3, 3, 1008, 8, "1024 dwords: spills of exactly 1, 2, 3 dwords at offsets 4, 8, 12, none at 0"),
    ("u8", 3, 3, 1040, 7, "1054 dwords: the right border lies in the second workgroup, the left one in the first"),
    ("f32", 3, 3, 339, 1, "1023 dwords, odd: spill-only second block, the shift rotates from row to row"),
    ("f32", 3, 3, 330, 8, "1038 dwords: the right border run is split between the two workgroups"),
]


def pad_cell(case):
    px, n, h, w, p, _ = case
    return {"name": "pad", "px": px, "n": n, "bx": 2, "by": h + 2 * p}


# (px, n, H, W, y0, x0, ch, cw, what it is for): the window inside a larger image on all four sides, x0 odd (source and destination
# disagree about where the 16-byte groups lie), ch = 6 (two row groups, the second ragged)
CROP_CASES = [
    ("u8", 3, 9, 1030, 2, 3, 6, 1022, "spill-only second block"),
    ("u8", 3, 9, 1029, 1, 1, 6, 1023, "odd row length: the shift rotates"),
    ("u8", 3, 8, 1033, 1, 5, 6, 1024, "spills of 1, 2, 3 dwords at offsets 4, 8, 12"),
    ("u8", 3, 9, 1060, 2, 3, 6, 1054, "whole groups in the second block"),
    ("f32", 3, 9, 347, 2, 3, 6, 341, "1023 dwords: spill-only second block, rotating shift"),
    ("f32", 3, 8, 350, 1, 1, 6, 346, "1038 dwords: whole groups in the second block"),
]


def crop_cell(case):
    px, n = case[0], case[1]
    return {"name": "crop", "px": px, "n": n, "bx": 2, "by": 2}


# ---- merge and bleed -------------------------------------------------------------------------------------------------------------------
# (factor, n, h, w, what it is for): h = 6 is two groups of four LR rows, the second ragged
MERGE_CASES = [
    (4, 3, 6, 70, "OW = 280: whole groups in the second block at a shifted address"),
    (4, 3, 6, 64, "OW = 256: the second block holds only the 1, 2, 3 pixels an offset of 4, 8, 12 pushes right"),
    (2, 3, 6, 128, "OW = 256 at factor 2"),
    (3, 3, 6, 85, "OW = 255, odd: the shift rotates from row to row"),
]


def merge_cell(case):
    f, n = case[0], case[1]
    return {"name": "merge", "px": "u8", "n": n, "bx": 2, "by": 2, "f": f}


def merge_images(case):
    """The LR batch (random colours, random alpha) and the output the merge writes into (random bytes, whose colours must stay)."""
    f, n, h, w, _ = case
    rng = np.random.default_rng(1000 * f + w)
    return rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8), rng.integers(0, 256, (n, f * h, f * w, 4), dtype=np.uint8)


BLEED_CASE = (3, 33, 65, 16)   # n, h, w, radius: 3 x 2 tiles of 32 x 32 per image
BLEED_CELL = {"name": "bleed", "px": "u8", "n": 3, "bx": 3, "by": 2}


def bleed_images():
    n, h, w, radius = BLEED_CASE
    return np.stack([alpha_ref.alpha_pattern(("sparse", "dense", "corner")[i], h, w, radius, 40 + i) for i in range(n)])


# ---- resize --------------------------------------------------------------------------------------------------------------------------
def rgba_batch(seed, n, h, w):
    """Seeded RGBA noise, the left half dark (bytes below 16: the transfer function's linear branch), as tests/test_gpu_resize.py's."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    px[:, :, : w // 2, :3] //= 16
    return px


def as_f32(px):
    """byte / 255 as f32: what an f32 input of those pixels holds"""
    return px[..., :3].astype(np.float32) / np.float32(255.0)


# ((h, w), (oh, ow), filters, the resize_h cell, the resize_v cell), all at n = 2.  by of resize_h counts groups of the batch's n h rows:
# with four rows to a group and h no multiple of 4, a group straddles the two images.
RESIZE_N = 2
RESIZE_CASES = [
    # the staged form, four rows a group: rows 4..7 of the 12 are image 0's last two and image 1's first two
    ((6, 900), (5, 600), ("triangle", "catrom", "lanczos3"), {"form": "staged4", "bx": 3, "by": 3}, {"bx": 3, "by": 2}),
    # ... for a box, which is staged only where it does not shrink; resize_v: three row groups of 9 rows, two column blocks
    ((3, 100), (9, 300), ("box", "triangle", "catrom", "lanczos3"), {"form": "staged4", "bx": 2, "by": 2}, {"bx": 2, "by": 3}),
    # one row's run fits the LDS, four do not
    ((5, 2100), (3, 520), ("triangle", "catrom", "lanczos3"), {"form": "staged1", "bx": 3, "by": 10}, {"bx": 3, "by": 1}),
    # not even one row's run fits (a scale of 14)
    ((3, 4200), (3, 300), ("triangle", "catrom", "lanczos3"), {"form": "direct", "bx": 2, "by": 2}, {"bx": 2, "by": 1}),
    # a box that shrinks reads nothing twice: direct at any scale
    ((2, 1000), (2, 300), ("box",), {"form": "direct", "bx": 2, "by": 1}, {"bx": 2, "by": 1}),
    ((6, 900), (5, 600), ("box",), {"form": "direct", "bx": 3, "by": 3}, {"bx": 3, "by": 2}),
    # resize_v: two column blocks, two row groups with a ragged second, taps that shrink
    ((9, 300), (6, 300), ("triangle", "catrom", "lanczos3"), {"form": "staged4", "bx": 2, "by": 5}, {"bx": 2, "by": 2}),
    ((9, 300), (6, 300), ("box",), {"form": "direct", "bx": 2, "by": 5}, {"bx": 2, "by": 2}),   # (a box at scale 1 is "a box that shrinks")
]
RESIZE_KINDS = (("rgba8", "rgba8"), ("f32", "f32"), ("rgba8", "f32"), ("f32", "rgba8"))   # (input, output), every pair in every case
# ... but RGBA8 output is not asked of the runs below.  Their restatement is TIED: means of two or four bytes (a box that shrinks, a
# triangle at a scale of 1.5, a few sRGB-space cases on the dark half's bytes 0 .. 15) put 0.1 % .. 28 % of its values exactly ON a
# rounding boundary -- within 255 x 1e-7, where an untied value falls 5e-5 of the time -- and which byte stands there is decided by the
# last bit of an f32 sum.  The u8 rule's cap on the differing share is a condition on the inputs (tests/test_operator_grids_cpu.py holds
# this list to the restatement, and the runs that stay to a share near a boundary below 1e-3); these runs keep their f32 output.
TIE_EPS, TIE_SHARE = 1e-7, 1e-3
RESIZE_TIED = {
    ((6, 900), (5, 600), "triangle", True), ((3, 100), (9, 300), "catrom", True), ((3, 4200), (3, 300), "triangle", True),
    ((2, 1000), (2, 300), "box", False), ((2, 1000), (2, 300), "box", True), ((6, 900), (5, 600), "box", False), ((6, 900), (5, 600), "box", True),
    ((9, 300), (6, 300), "triangle", False), ((9, 300), (6, 300), "triangle", True), ((9, 300), (6, 300), "catrom", True),
    ((9, 300), (6, 300), "box", False), ((9, 300), (6, 300), "box", True),
}
EPS_GRID = 1.2e-6   # the worst f32 error of the grid cases on an MI355X, rounded up (1.093e-6 measured, 2026-10-20)


def resize_kinds(run):
    """The (input, output) kinds a run is held to: all four, without RGBA8 output where the restatement is tied."""
    return tuple(k for k in RESIZE_KINDS if k[1] == "f32" or run[:4] not in RESIZE_TIED)


def resize_runs():
    """[(shape, size, filter, srgb_space, h_cell, v_cell)]: every case under every filter it lists, in linear light and in sRGB space."""
    return [(shape, size, name, srgb_space, h_cell, v_cell)
            for shape, size, names, h_cell, v_cell in RESIZE_CASES for name in names for srgb_space in (False, True)]


def resize_seed(shape, size):
    return shape[0] * 100003 + shape[1] * 1009 + size[0] * 31 + size[1]


def resize_cells(run, in_kind, out_kind):
    shape, size, name, srgb_space, h_cell, v_cell = run
    px = {"rgba8": "u8", "f32": "f32"}
    return (dict(h_cell, name="resize_h", px=px[in_kind], n=RESIZE_N), dict(v_cell, name="resize_v", px=px[out_kind], n=RESIZE_N))


def resize_rounded(x, size, name, srgb_space):
    """resize_ref.resize with its samples rounded to f32 after each pass (the linearised input, the horizontal pass, the vertical pass):
    what the f32 formats of the kernels' three stores cost, whatever order they add in."""
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = np.asarray(x, dtype=np.float64)
    oh, ow = size
    if not srgb_space:
        x = r32(resize_ref.srgb_to_linear(x))
    y = r32(resize_ref.resize_axis(r32(resize_ref.resize_axis(x, -2, ow, name)), -3, oh, name))
    return y if srgb_space else resize_ref.linear_to_srgb(y)


_refs = {}


def reference(key, make_input, size, name, srgb_space):
    """The f64 restatement of the f32 batch make_input() gives, computed once per key and left unchanged."""
    k = (key, size, name, srgb_space)
    if k not in _refs:
        ref = resize_ref.resize(np.asarray(make_input(), dtype=np.float32).astype(np.float64), size, name, srgb_space)
        ref.setflags(write=False)
        _refs[k] = ref
    return _refs[k]


def grid_reference(run):
    shape, size, name, srgb_space = run[:4]
    return reference(("grid",) + shape, lambda: as_f32(rgba_batch(resize_seed(shape, size), RESIZE_N, *shape)), size, name, srgb_space)


def near_boundary(v, eps):
    """Mask of the restatement values within 255 eps (in levels) of a rounding boundary that separates two bytes: 255 v + 0.5 = k,
    k = 1 .. 255 (a value beyond them is clamped whichever side it falls)."""
    frac = 255.0 * np.asarray(v, dtype=np.float64) + 0.5
    k = np.clip(np.round(frac), 1, 255)
    return np.abs(frac - k) < 255.0 * eps


# ---- resize on f32 pixels outside byte / 255 (the network's unclamped output is the real f32 input, through sr_upscale_rgba8_sized) ----
CLASS_SHAPES = [((7, 9), (3, 4)), ((5, 31), (8, 50)), ((9, 257), (5, 129))]
CLASS_NAMES = ("dark_f32", "edge_f32", "wide_f32")
CLASS_N = 2
# Seeds per class.  The wide_f32 seed is the one of 13 .. 139 with the fewest restatement values at a rounding boundary: the RGBA8-output
# test's cap on the differing share is a condition on the inputs (tests/test_operator_grids_cpu.py), and values that do not leave
# [0, 1] fall within 255 e of a boundary 2 x 255 e of the time -- about the 5e-4 that condition allows, so most seeds miss it.
CLASS_SEED = {"dark_f32": 11, "edge_f32": 12, "wide_f32": 126}
# (class, filter, srgb_space) that the conditioning gate of tests/test_operator_grids_cpu.py turned away: none
CLASS_DROPPED = ()
EPS_U8 = 1.8e-6   # the worst f32 error of the wide_f32 cases on an MI355X, rounded up (test_resize_on_f32_classes printed 1.795e-6, 2026-10-20)


def class_input(cls, shape):
    return pc.make(cls, CLASS_SEED[cls] * 1000 + 7 * shape[0] + shape[1], CLASS_N, *shape)


def class_runs(classes=CLASS_NAMES):
    return [(cls, shape, size, name, srgb_space) for cls in classes for shape, size in CLASS_SHAPES for name in resize_ref.FILTERS
            for srgb_space in (False, True) if (cls, name, srgb_space) not in CLASS_DROPPED]


def class_reference(run):
    cls, shape, size, name, srgb_space = run
    return reference((cls,) + shape, lambda: class_input(cls, shape), size, name, srgb_space)


def class_bar(want):
    """TOL times max(1, |want|.max()): the form tests/test_gpu_parity.py uses for values that leave the unit range"""
    return TOL * max(1.0, float(np.abs(want).max()))
