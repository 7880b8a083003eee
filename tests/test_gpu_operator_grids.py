"""The pixel operators around the network on the grid cells their other tests never reach (tests/operator_grid_cases.py): two and three
column blocks together with a batch and several row groups, the last column block holding only the dwords a misaligned row pushes
right, every form of the resampler's horizontal pass with row groups that straddle two images, resize_v's second column block on the
second image -- and the resampler on f32 pixels outside byte / 255.  Every call is followed by an assertion on the plan record
(Engine.last_plan()["ops"]) that the intended cell ran: the record, not the case table, decides what a shape reaches.  Pad, crop, bleed
and merge byte for byte against border_ref / alpha_ref; resize at the bars of tests/test_gpu_resize.py.  Buffers lie at byte offsets 0, 4,
8 and 12 of a larger 16-byte aligned allocation filled with 0xA5, whose guard bytes are checked afterwards."""
import numpy as np
import pytest

import alpha_ref
import border_ref
import operator_grid_cases as og
import resize_ref
from test_gpu_border import guards_intact, offset_view, same_bytes
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

SEEN = {}   # operator -> {(n > 1, by > 1, bx > 1, offset, form or factor)}: what the records of this module's calls showed
HELD = set()   # the operators whose grid test has run: test_coverage_table holds those to the full cell at every offset


@pytest.fixture(scope="module")
def engines():
    import rusty_sr_amd as r
    made = {}

    def get(factor=3):
        if factor not in made:
            # the operators use no parameters; the parameter-free graph exists at factor 3 only
            made[factor] = r.Engine(graph="bilinear") if factor == 3 else r.Engine(synthetic_params(factor, 100 + factor), factor=factor)
        return made[factor]
    yield get
    for e in made.values():
        e.close()


def ran(e, offset, *cells):
    """The ops of the engine's last call are exactly `cells` (dicts of the fields each must show), in order."""
    ops = e.last_plan()["ops"]
    assert len(ops) == len(cells), (ops, cells)
    for op, want in zip(ops, cells):
        assert op["count"] == 1 and og.cell_mismatch(op, want) == {}, (op, want)
        SEEN.setdefault(op["name"], set()).add((op["n"] > 1, op["by"] > 1, op["bx"] > 1, offset, op.get("form", op.get("f", "-"))))


def upload(arr, offset):
    """arr in device memory `offset` bytes into a guarded allocation -> (view, whole)"""
    import torch
    view, whole = offset_view(arr.shape, arr.dtype, offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return view, whole


def nbytes(arr):
    return arr.size * arr.dtype.itemsize


# ---- pad and crop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(og.PAD_CASES)), ids=[f"{c[0]}-{c[3]}+2x{c[4]}" for c in og.PAD_CASES])
def test_pad_across_two_workgroups_of_a_batch(engines, k):
    import torch
    e = engines()
    case = og.PAD_CASES[k]
    px, n, h, w, p, _ = case
    img = og.dword_image(k, px, n, h, w)
    want = {mode: border_ref.pad(img, mode, p) for mode in border_ref.MODES}
    for offset in og.OFFSETS:
        src, src_whole = upload(img, (offset + 4) % 16)
        for mode in border_ref.MODES:
            dst, whole = offset_view(want[mode].shape, img.dtype, offset)
            e.pad(src, mode, p, out=dst)
            ran(e, offset, og.pad_cell(case))
            torch.cuda.synchronize()
            assert same_bytes(dst.cpu().numpy(), want[mode]), (case, mode, offset)
            assert guards_intact(whole, offset, nbytes(want[mode])), (case, mode, offset)
        assert guards_intact(src_whole, (offset + 4) % 16, nbytes(img)) and same_bytes(src.cpu().numpy(), img)
    HELD.add("pad")


@pytest.mark.parametrize("k", range(len(og.CROP_CASES)), ids=[f"{c[0]}-{c[7]}" for c in og.CROP_CASES])
def test_crop_across_two_workgroups_of_a_batch(engines, k):
    import torch
    e = engines()
    case = og.CROP_CASES[k]
    px, n, H, W, y0, x0, ch, cw, _ = case
    img = og.dword_image(100 + k, px, n, H, W)
    want = border_ref.crop(img, y0, x0, ch, cw)
    for offset in og.OFFSETS:
        src, src_whole = upload(img, (offset + 8) % 16)
        dst, whole = offset_view(want.shape, img.dtype, offset)
        e.crop(src, y0, x0, ch, cw, out=dst)
        ran(e, offset, og.crop_cell(case))
        torch.cuda.synchronize()
        assert same_bytes(dst.cpu().numpy(), want), (case, offset)
        assert guards_intact(whole, offset, nbytes(want)), (case, offset)
        assert guards_intact(src_whole, (offset + 8) % 16, nbytes(img)) and same_bytes(src.cpu().numpy(), img)
    HELD.add("crop")


# ---- merge and bleed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(og.MERGE_CASES)), ids=[f"f{c[0]}-w{c[3]}" for c in og.MERGE_CASES])
def test_merge_across_two_workgroups_of_a_batch(engines, k):
    import torch
    case = og.MERGE_CASES[k]
    f = case[0]
    e = engines(f)
    lr, out = og.merge_images(case)
    want = out.copy()
    want[..., 3] = alpha_ref.up_alpha(lr[..., 3], f)
    assert (want[..., 3] != out[..., 3]).any()
    for offset in og.OFFSETS:
        src, _ = upload(lr, (offset + 4) % 16)
        dst, whole = upload(out, offset)
        e.merge_alpha(src, dst)
        ran(e, offset, og.merge_cell(case))
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        np.testing.assert_array_equal(got[..., :3], out[..., :3], err_msg=f"colours, {case}, offset {offset}")
        assert same_bytes(got, want), (case, offset)
        assert guards_intact(whole, offset, nbytes(want)), (case, offset)
    HELD.add("merge")


def test_bleed_of_a_batch_over_its_tiles(engines):
    import torch
    e = engines()
    radius = og.BLEED_CASE[3]
    px = og.bleed_images()
    want = alpha_ref.bleed(px, radius)
    for offset in og.OFFSETS:
        src, _ = upload(px, (offset + 4) % 16)
        dst, whole = offset_view(px.shape, np.uint8, offset)
        e.bleed(src, radius, out=dst)
        ran(e, offset, og.BLEED_CELL)
        torch.cuda.synchronize()
        assert same_bytes(dst.cpu().numpy(), want), offset
        assert guards_intact(whole, offset, nbytes(want)), offset
    HELD.add("bleed")


# ---- resize: every form of the horizontal pass and the vertical pass beyond one column block, in a batch ---------------------------------
class U8Pool:
    """tests/test_gpu_resize.py's u8 rule: |d| <= 1 and every differing byte within 255 x 1e-4 of a rounding knife-edge of the restatement,
    alpha 255, checked per call; the differing share below 1e-3, pooled over the calls of a test."""

    def __init__(self):
        self.differing = self.total = 0

    def add(self, got, v, where):
        want = resize_ref.quantise(v)
        assert got.shape == want.shape and (got[..., 3] == 255).all(), where
        d = got[..., :3].astype(int) - want[..., :3].astype(int)
        assert np.abs(d).max() <= 1, where
        if (d != 0).any():
            frac = 255.0 * v + 0.5
            assert np.abs(frac - np.round(frac))[d != 0].max() < 255 * 1e-4, ("u8 mismatch away from a rounding knife-edge", where)
        self.differing += int((d != 0).sum())
        self.total += d.size

    def check(self):
        print(f"differing bytes: {self.differing} of {self.total}")
        assert self.total > 0 and self.differing / self.total < 1e-3


def resize_call(e, x, size, out_kind, name, srgb_space, offset, cells):
    """resize_dev of the numpy batch x (u8 RGBA or f32 RGB), input and output at offsets; the record, the guards, the untouched input."""
    import torch
    n = x.shape[0]
    out_dtype, out_ch = (np.uint8, 4) if out_kind == "rgba8" else (np.float32, 3)
    src, src_whole = upload(x, (offset + 12) % 16)
    dst, whole = offset_view((n,) + size + (out_ch,), out_dtype, offset)
    e.resize_dev(src, size, out_kind, name, srgb_space, out=dst)
    ran(e, offset, *cells)
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert guards_intact(whole, offset, nbytes(got)) and guards_intact(src_whole, (offset + 12) % 16, nbytes(x))
    assert same_bytes(src.cpu().numpy(), x)
    return got


GRID_RUNS = og.resize_runs()


@pytest.mark.parametrize("form", ["staged4", "staged1", "direct"])
def test_resize_forms_in_a_batch_beyond_one_column_block(engines, form):
    """Every (input, output) kind of every case of the form (RGBA8 output where the restatement is not tied: operator_grid_cases.RESIZE_TIED),
    held to the restatement of EACH image of the batch."""
    e = engines()
    pool, worst, calls = U8Pool(), 0.0, 0
    for run in GRID_RUNS:
        shape, size, name, srgb_space, h_cell, v_cell = run
        if h_cell["form"] != form:
            continue
        px = og.rgba_batch(og.resize_seed(shape, size), og.RESIZE_N, *shape)
        want = og.grid_reference(run)
        assert not np.array_equal(want[0], want[1])
        for in_kind, out_kind in og.resize_kinds(run):
            offset = og.OFFSETS[calls % 4]
            calls += 1
            x = px if in_kind == "rgba8" else og.as_f32(px)
            got = resize_call(e, x, size, out_kind, name, srgb_space, offset, og.resize_cells(run, in_kind, out_kind))
            where = (shape, size, name, srgb_space, in_kind, out_kind, offset)
            if out_kind == "f32":
                err = [float(np.abs(got[i] - want[i]).max()) for i in range(og.RESIZE_N)]
                print(f"{name} srgb_space={srgb_space} {in_kind} {shape}->{size} @{offset}: max abs {err[0]:.3e} {err[1]:.3e}")
                worst = max(worst, *err)
                assert got.shape == want.shape and max(err) < og.TOL, where
            else:
                pool.add(got, want, where)
    assert calls >= 8
    print(f"{form}: worst f32 error {worst:.3e} over {calls} calls")
    pool.check()
    HELD.update(("resize_h",) if form == "staged1" else ("resize_h", "resize_v"))   # (no staged1 case has two row groups of resize_v)


# ---- resize on f32 pixels outside byte / 255 -----------------------------------------------------------------------------------------
CLASS_CELLS = ({"name": "resize_h", "px": "f32", "n": og.CLASS_N}, {"name": "resize_v", "px": "f32", "n": og.CLASS_N})


@pytest.mark.parametrize("cls", og.CLASS_NAMES)
def test_resize_on_f32_classes(engines, cls):
    """f32 in, f32 out, all four filters, linear light and sRGB space: srgb_to_linear_fast below 0, above 1 and around its branch point.
    Bar: TOL x max(1, |want|.max()).  Prints the worst error (absolute, and as a share of the bar): for wide_f32 that is the e of
    tests/test_operator_grids_cpu.py's boundary condition."""
    e = engines()
    worst = worst_share = 0.0
    for k, run in enumerate(og.class_runs((cls,))):
        _, shape, size, name, srgb_space = run
        want = og.class_reference(run)
        got = resize_call(e, og.class_input(cls, shape), size, "f32", name, srgb_space, og.OFFSETS[k % 4], CLASS_CELLS)
        err, bar = float(np.abs(got - want).max()), og.class_bar(want)
        print(f"{cls} {name} srgb_space={srgb_space} {shape}->{size}: max abs {err:.3e}, bar {bar:.3e}")
        worst, worst_share = max(worst, err), max(worst_share, err / bar)
        assert got.shape == want.shape and err < bar, (run, err, bar)
    print(f"{cls}: worst f32 error {worst:.3e} ({worst_share:.3f} of its bar)")


def test_resize_wide_f32_to_rgba8(engines):
    """The quantiser behind values that leave [0, 1]: the u8 rule on wide_f32, pooled over the cases."""
    e = engines()
    pool = U8Pool()
    cells = (CLASS_CELLS[0], dict(CLASS_CELLS[1], px="u8"))
    for k, run in enumerate(og.class_runs(("wide_f32",))):
        _, shape, size, name, srgb_space = run
        got = resize_call(e, og.class_input("wide_f32", shape), size, "rgba8", name, srgb_space, og.OFFSETS[k % 4], cells)
        pool.add(got, og.class_reference(run), run)
    pool.check()


# ---- the composed calls write the lines of the launches they queue, in order; the plain calls none ---------------------------------------
def test_composed_calls_record_their_operators(params):
    import torch
    import rusty_sr_amd as r
    e = r.Engine(params["imagenet"])
    try:
        n, h, w, p, f = 2, 9, 11, 8, 3
        px = og.rgba_batch(3, n, h, w)
        px[..., 3] = alpha_ref.alpha_pattern("dense", h, w, 8, 1)[..., 3]
        t = torch.from_numpy(px).cuda()
        one = {"n": n, "bx": 1}
        bleed, merge = dict(one, name="bleed", px="u8", by=1), dict(one, name="merge", px="u8", by=3, f=f)

        def pad(kind):
            return dict(one, name="pad", px=kind, by=h + 2 * p)

        def crop(kind):
            return dict(one, name="crop", px=kind, by=-(-f * h // 4))

        e.upscale_rgba8_border_dev(t, "wrap", p, bleed=8)
        ran(e, 0, bleed, pad("u8"), crop("u8"), merge)
        assert e.last_plan()["launches"]   # ... around the network's own lines
        e.upscale_rgba8_border_dev(t, "mirror", p)
        ran(e, 0, pad("u8"), crop("u8"))
        e.upscale_rgba8_border(px, "replicate", p, bleed=0)   # the host call; a radius of 0 bleeds nothing and launches nothing
        ran(e, 0, pad("u8"), crop("u8"), merge)
        e.upscale_f32_border_dev(torch.from_numpy(r.img_to_data(px)).cuda(), "wrap", p)
        ran(e, 0, pad("f32"), crop("f32"))
        e.upscale_rgba8_alpha_dev(t, 8)
        ran(e, 0, bleed, merge)
        e.upscale_rgba8_alpha(px, 8)
        ran(e, 0, bleed, merge)
        sized = (dict(one, name="resize_h", px="f32", by=-(-n * f * h // 4), form="staged4"), dict(one, name="resize_v", px="u8", by=5))
        e.upscale_rgba8_sized_dev(t, (20, 40))
        ran(e, 0, *sized)
        e.upscale_rgba8_sized(px, (20, 40))
        ran(e, 0, *sized)
        assert e.last_plan()["launches"]
        # the plain calls write no such line, and clear the ones before
        e.upscale_rgba8_dev(t)
        assert e.last_plan()["ops"] == [] and e.last_plan()["launches"]
        e.upscale_rgba8(px)
        assert e.last_plan()["ops"] == []
        torch.cuda.synchronize()
    finally:
        e.close()


# ---- what ran ------------------------------------------------------------------------------------------------------------------------
def test_coverage_table():
    """Prints, per operator, the (n > 1, by > 1, bx > 1, offset, form / factor) cells the records of this module showed, and holds each
    operator whose grid test ran to the cell the module is for: batch, several row groups and several column blocks at once, at every
    offset."""
    lines = ["| operator | n>1 | by>1 | bx>1 | offset | form / f |"]
    for name in sorted(SEEN):
        for cell in sorted(SEEN[name], key=str):
            lines.append(f"| {name} | " + " | ".join(str(v) for v in cell) + " |")
    print("\n" + "\n".join(lines))
    for name in sorted(HELD):
        full = {c[3] for c in SEEN[name] if c[0] and c[1] and c[2]}
        assert full == set(og.OFFSETS), (name, sorted(SEEN[name], key=str))
