"""The case tables of tests/operator_grid_cases.py on the restatements alone (border_ref, alpha_ref, resize_ref), without a GPU: the
cases build, the images of a batch differ, every resize case is well enough conditioned for the bar tests/test_gpu_operator_grids.py
holds it to, and parse_plan reads the `op` lines those tests assert on.  A case that fails a gate leaves its table (and the table says
which); its bar is not widened."""
import numpy as np
import pytest

import alpha_ref
import border_ref
import operator_grid_cases as og
import resize_ref


def differ(batch):
    return all(not np.array_equal(batch[i].view(np.uint8), batch[j].view(np.uint8)) for i in range(len(batch)) for j in range(i))


# ---- the tables build --------------------------------------------------------------------------------------------------------------
def test_pad_and_crop_cases_build():
    kinds = set()
    for k, case in enumerate(og.PAD_CASES):
        px, n, h, w, p, _ = case
        img = og.dword_image(k, px, n, h, w)
        assert differ(img) and n >= 2
        for mode in border_ref.MODES:
            out = border_ref.pad(img, mode, p)
            assert out.shape == (n, h + 2 * p, w + 2 * p, img.shape[-1])
        cell = og.pad_cell(case)
        assert cell["bx"] >= 2 and cell["by"] >= 2 and cell["n"] == n
        row_dwords = (w + 2 * p) * (1 if px == "u8" else 3)
        if row_dwords % 4:
            kinds.add(px)
    assert kinds == {"u8", "f32"}   # a row length that rotates the shift from row to row, per pixel kind
    for k, case in enumerate(og.CROP_CASES):
        px, n, H, W, y0, x0, ch, cw, _ = case
        img = og.dword_image(100 + k, px, n, H, W)
        assert differ(img) and n >= 2 and x0 % 2 == 1 and ch == 6
        assert y0 > 0 and x0 > 0 and y0 + ch < H and x0 + cw < W   # inside on all four sides
        assert differ(border_ref.crop(img, y0, x0, ch, cw))


def test_merge_and_bleed_cases_build():
    for case in og.MERGE_CASES:
        f, n, h, w, _ = case
        lr, out = og.merge_images(case)
        assert differ(lr) and differ(out) and differ(alpha_ref.up_alpha(lr[..., 3], f))
        assert out.shape == (n, f * h, f * w, 4) and h == 6 and n == 3
    assert {(c[0] * c[3]) % 256 for c in og.MERGE_CASES} >= {0, 24, 255}   # OW = 256 (spill only), 280, 255
    px = og.bleed_images()
    assert differ(px)
    bled = alpha_ref.bleed(px, og.BLEED_CASE[3])
    assert any(not np.array_equal(bled[i], px[i]) for i in range(len(px)))   # the bleed has something to do


def test_resize_tables_build():
    runs = og.resize_runs()
    forms = {}
    for run in runs:
        shape, size, name, srgb_space, h_cell, v_cell = run
        assert differ(og.rgba_batch(og.resize_seed(shape, size), og.RESIZE_N, *shape))
        assert shape[0] <= 10 and size[0] <= 10   # the restatement is a Python loop
        forms.setdefault(h_cell["form"], set()).add(srgb_space)
        assert h_cell["bx"] >= 2 and v_cell["bx"] >= 2
    assert forms == {"staged4": {False, True}, "staged1": {False, True}, "direct": {False, True}}
    # resize_v with two column blocks, two row groups and a ragged last group; resize_h groups that straddle the two images
    assert any(v["by"] >= 2 and size[0] % 4 for _, size, _, _, _, v in runs)
    assert any(h["form"] != "staged1" and shape[0] % 4 and h["by"] >= 2 for shape, _, _, _, h, _ in runs)
    for cls in og.CLASS_NAMES:
        for shape, _ in og.CLASS_SHAPES:
            assert differ(og.class_input(cls, shape))
    assert len(og.class_runs()) + len(og.CLASS_DROPPED) * len(og.CLASS_SHAPES) == len(og.CLASS_NAMES) * len(og.CLASS_SHAPES) * 4 * 2


# ---- conditioning: the f32 formats of the kernels' stores must cost less than a quarter of the bar ------------------------------------
def test_grid_cases_are_well_conditioned():
    worst = 0.0
    for run in og.resize_runs():
        shape, size, name, srgb_space = run[:4]
        x = og.as_f32(og.rgba_batch(og.resize_seed(shape, size), og.RESIZE_N, *shape))
        err = float(np.abs(og.resize_rounded(x, size, name, srgb_space) - og.grid_reference(run)).max())
        worst = max(worst, err)
        assert err <= og.GATE * og.TOL, (run[:4], err)
    print(f"grid cases: f32-rounded restatement within {worst:.3e} of the f64 one (gate {og.GATE * og.TOL:.1e})")


def test_grid_cases_with_rgba8_output_keep_clear_of_the_rounding_boundaries():
    """The u8 rule caps the differing share at 1e-3, pooled over a test's calls.  A byte can differ only where the restatement lies within
    the kernel's f32 error of a rounding boundary, so the cap is a condition on the inputs: over the runs of each form that are asked for
    RGBA8 output, fewer than 1e-3 of the restatement values may lie within 255 e of a boundary, e = EPS_GRID (the worst f32 error the GPU
    test printed for these cases; untied values fall there 2 x 255 e = 6e-4 of the time).  RESIZE_TIED is exactly the runs whose
    restatement stands ON a boundary far more often than that."""
    tied, pooled = set(), {}
    for run in og.resize_runs():
        v = og.grid_reference(run)
        if og.near_boundary(v, og.TIE_EPS).mean() > og.TIE_SHARE:
            tied.add(run[:4])
        if any(out == "rgba8" for _, out in og.resize_kinds(run)):
            acc = pooled.setdefault(run[4]["form"], [0, 0])
            acc[0] += int(og.near_boundary(v, og.EPS_GRID).sum())
            acc[1] += v.size
    assert tied == og.RESIZE_TIED, (tied ^ og.RESIZE_TIED)
    assert set(pooled) == {"staged4", "staged1", "direct"}   # every form keeps RGBA8 output, in linear light and in sRGB space
    for form in pooled:
        spaces = {run[3] for run in og.resize_runs() if run[4]["form"] == form and run[:4] not in og.RESIZE_TIED}
        assert spaces == {False, True}, form
    for form, (near, total) in pooled.items():
        print(f"{form}: {near} of {total} restatement values within 255 x {og.EPS_GRID:g} of a rounding boundary ({near / total:.3e})")
        assert near / total < 1e-3, form
    # resize_v with RGBA8 output in a second column block, two row groups, the last ragged: still there
    assert any(run[5]["by"] >= 2 and run[5]["bx"] >= 2 and run[1][0] % 4 and run[:4] not in og.RESIZE_TIED for run in og.resize_runs())


@pytest.mark.parametrize("cls", og.CLASS_NAMES)
def test_class_cases_are_well_conditioned(cls):
    """The restatement with its samples rounded to f32 after each pass must lie within a quarter of the case's bar of the f64 result."""
    worst = 0.0
    for run in og.class_runs((cls,)):
        _, shape, size, name, srgb_space = run
        want = og.class_reference(run)
        err = float(np.abs(og.resize_rounded(og.class_input(cls, shape), size, name, srgb_space) - want).max())
        bar = og.class_bar(want)
        worst = max(worst, err / bar)
        assert err <= og.GATE * bar, (run, err, bar)
    print(f"{cls}: f32-rounded restatement within {worst:.3f} of the bar at the worst (gate {og.GATE})")


def test_classes_reach_what_they_are_for():
    """dark_f32 and edge_f32 stand on both sides of SrgbToLinear's branch point, wide_f32 below 0 and above 1; the wide outputs leave
    the unit range on both sides too, so that the bar's max(1, |want|) and the quantiser's clamp are exercised."""
    shape = og.CLASS_SHAPES[-1][0]
    for cls in ("dark_f32", "edge_f32"):
        x = og.class_input(cls, shape)
        assert (x <= 0.04045).any() and (x > 0.04045).any()
    x = og.class_input("wide_f32", shape)
    assert x.min() < 0 and x.max() > 1
    want = og.class_reference(("wide_f32", *og.CLASS_SHAPES[1], "lanczos3", False))
    assert want.min() < 0 and want.max() > 1


def test_wide_cases_keep_clear_of_the_rounding_boundaries():
    """The RGBA8-output test on wide_f32 caps the differing share at 1e-3 (tests/test_gpu_resize.py's u8 rule).  That cap is a condition
    on the inputs, not a measurement: a byte can differ only where the restatement lies within the kernel's error of a rounding boundary,
    so the share of restatement values within 255 e of one must stay below 5e-4, pooled over the cases, for the chosen seed.
    e = operator_grid_cases.EPS_U8 = 1.8e-6: tests/test_gpu_operator_grids.py::test_resize_on_f32_classes[wide_f32] printed a worst f32
    error of 1.795e-6 for these cases and this seed on an MI355X on 2026-10-20 (24 of 50736 values, 4.7e-4, stay within 255 x 2e-6 too)."""
    near = total = 0
    for run in og.class_runs(("wide_f32",)):
        v = og.class_reference(run)
        near += int(og.near_boundary(v, og.EPS_U8).sum())
        total += v.size
    print(f"wide_f32: {near} of {total} restatement values within 255 x {og.EPS_U8:g} of a rounding boundary ({near / total:.3e})")
    assert near / total < 5e-4


# ---- the record ----------------------------------------------------------------------------------------------------------------------
def test_parse_plan_reads_op_lines():
    from rusty_sr_amd.engine import parse_plan
    text = ("op name=bleed px=u8 n=3 bx=3 by=2\n"
            "op name=pad px=f32 n=3 bx=2 by=19\n"
            "fork 0\n"
            "launch st=0 form=first ty8=1 ty4=0 grid=4 prec=f32 f=3 img=u8 out=u8 ch=4 x2\n"
            "op name=merge px=u8 n=3 bx=2 by=2 f=4\n"
            "op name=resize_h px=f32 n=2 bx=3 by=10 form=staged1 x2\n"
            "op name=resize_v px=u8 n=2 bx=2 by=3\n")
    rec = parse_plan(text)
    assert rec["ops"] == [
        {"name": "bleed", "px": "u8", "n": 3, "bx": 3, "by": 2, "count": 1},
        {"name": "pad", "px": "f32", "n": 3, "bx": 2, "by": 19, "count": 1},
        {"name": "merge", "px": "u8", "n": 3, "bx": 2, "by": 2, "f": 4, "count": 1},
        {"name": "resize_h", "px": "f32", "n": 2, "bx": 3, "by": 10, "form": "staged1", "count": 2},
        {"name": "resize_v", "px": "u8", "n": 2, "bx": 2, "by": 3, "count": 1},
    ]
    assert rec["fork"] == [(False, 0, 0)] and len(rec["launches"]) == 1 and rec["launches"][0]["count"] == 2
    assert og.cell_mismatch(rec["ops"][2], og.merge_cell(og.MERGE_CASES[0])) == {}
    assert og.cell_mismatch(rec["ops"][2], og.merge_cell(og.MERGE_CASES[2])) == {"f": (4, 2)}


def test_parse_plan_ignores_unknown_line_kinds():
    from rusty_sr_amd.engine import parse_plan
    rec = parse_plan("note something=else x3\nop name=crop px=u8 n=1 bx=1 by=1\nfuture a=1 b=2\n")
    assert rec == {"host": [], "fork": [], "launches": [], "aux": [], "ops": [{"name": "crop", "px": "u8", "n": 1, "bx": 1, "by": 1, "count": 1}]}
    assert parse_plan("") == {"host": [], "fork": [], "launches": [], "aux": [], "ops": []}
