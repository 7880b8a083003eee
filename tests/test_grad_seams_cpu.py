"""The premises of tests/test_gpu_grad_seams.py, on the f64 restatement alone (tests/grad_seam_cases.py, tests/grad_ref.py): the split
rules give the table's numbers and every impulse pixel is where the table says; one seam pixel's term is at least 100 bars of
assert_grad_close in the segments the seam's kernel sums; and without an impulse the restatement's gradient on its own rounded output
is below a thousandth of a bar.  A case that fails a gate here is a wrong case: the case changes, never the factor."""
import numpy as np
import pytest

import grad_ref
import grad_seam_cases as gs
from test_gpu_backprop import assert_grad_close

MARGIN = 100.0          # a seam pixel's term against the bar
RESIDUAL = 1e-3         # the impulse-free gradient against the bar
FIVES = ("conv0", "conv1", "conv2", "conv3")
BIAS_OF = {"conv0": "f_bias", "conv1": "l1_bias", "conv2": "l2_bias", "conv3": "l3_bias"}   # d_z of a layer = the gradient of that conv's output


def seg(g, f, name):
    off, n, _ = grad_ref.segments(f)[name]
    return g[off:off + n]


@pytest.mark.parametrize("case", sorted(gs.CASES))
def test_split_rules_give_the_table(case):
    c = gs.CASES[case]
    g = gs.split(c["n"], c["H"], c["W"])
    assert c["n"] * c["H"] * c["W"] == c["NP"]
    assert (g["wchunks"], g["wchunk"]) == c["w"] and (g["cchunks"], g["cchunk"]) == c["c"]
    assert (g["conv"], g["loss"]) == (c["conv"], c["loss"])


def test_the_table_says_what_the_issue_of_each_case_is():
    a, b, c, d = (gs.CASES[k] for k in "ABCD")
    assert a["w"][1] % 2 == 1 and divmod(a["w"][1], a["W"]) == (9, 16)                        # odd chunk, seam in mid-row
    hw = b["H"] * b["W"]
    assert b["w"][1] % 2 == 1 and hw < b["w"][1] < 2 * hw and (hw, 2 * hw) == (247, 494)        # chunk seam inside image 1
    assert 224 < hw < 256 and 480 < 2 * hw < 512                                                # image seams inside a wave of 32 pixels
    assert c["c"][0] == 2 and c["c"][1] % 4 == 1 and 3 * c["f"] ** 2 == 48                      # odd column-sum chunk, 1 mod 4; E > 32
    assert d["w"] == (128, 513) and -(-d["NP"] // 512) > 128 and d["NP"] - 127 * 513 == 470     # the cap; the last chunk
    assert d["NP"] < 262144                                                                     # (the cap on cchunks is not reached)


@pytest.mark.parametrize("row", gs.ROWS, ids=gs.row_id)
def test_every_impulse_pixel_is_where_the_table_says(row):
    case, _, _, px = row
    c = gs.CASES[case]
    g = gs.split(c["n"], c["H"], c["W"])
    for p, tags in px:
        assert tags <= gs.stands_on(p, g), (p, tags, gs.stands_on(p, g))
    # impulses of one call: beside the same seam, or far enough apart for disjoint cones
    at = [divmod(p % (c["H"] * c["W"]), c["W"]) + (p // (c["H"] * c["W"]),) for p, _ in px]
    for i in range(len(px)):
        for j in range(i + 1, len(px)):
            apart = max(abs(at[i][0] - at[j][0]), abs(at[i][1] - at[j][1]))
            assert abs(px[i][0] - px[j][0]) == 1 or at[i][2] != at[j][2] or apart >= gs.CONE, (px[i][0], px[j][0])


def test_rows_cover_every_seam_the_cases_are_for():
    have = {}
    for case, weights, linear, px in gs.ROWS:
        for p, tags in px:
            have.setdefault(case, set()).update(tags)
    assert {"wgrad:chunk:last", "wgrad:chunk:first", "wgrad:chunk:unpaired", "wgrad:chunk:midrow", "conv:workgroup:last",
            "conv:workgroup:first", "loss:partial:last", "loss:partial:first", "tail"} <= have["A"]
    assert {"image:seam:last", "image:seam:first", "image:lastrow", "image:firstrow", "conv:wave:last", "conv:wave:first",
            "wgrad:chunk:unpaired"} <= have["B"]
    assert {"colsum:chunk:last", "colsum:chunk:first", "wgrad:chunk:last", "wgrad:chunk:first"} <= have["C"]
    assert {"wgrad:capped", "colsum:chunk:last", "colsum:chunk:first", "tail", "wgrad:chunk:unpaired"} <= have["D"]
    for case, k in (("A", 1), ("B", 1), ("C", 2)):   # every weight-chunk seam of A - C
        w = gs.CASES[case]["w"][1]
        ps = {p for r in gs.ROWS if r[0] == case for p in gs.pixels(r)}
        assert all({s * w - 1, s * w} <= ps for s in range(1, k + 1))


def test_norm_bar_is_the_bar_of_assert_grad_close():
    f = 2
    rng = np.random.default_rng(1)
    want = rng.standard_normal(grad_ref.num_params(f))
    step = rng.standard_normal(want.size)
    for name, (off, n, _) in grad_ref.segments(f).items():
        d = np.zeros_like(want)
        d[off:off + n] = step[off:off + n] / np.linalg.norm(step[off:off + n]) * gs.norm_bar(want[off:off + n])
        assert_grad_close(want + 0.99 * d, want, f)
        with pytest.raises(AssertionError):
            assert_grad_close(want + 1.01 * d, want, f)


def test_parse_plan_reads_the_grad_line():
    from rusty_sr_amd.engine import parse_plan
    text = "grad n=1 h=19 w=31 conv=5 loss=3 wchunks=2 wchunk=295 cchunks=1 cchunk=589\n"
    assert parse_plan(text)["grad"] == [dict(gs.split(1, 19, 31), count=1)]
    two = parse_plan("op name=crop px=u8 n=1 bx=1 by=1\n" + text.rstrip() + " x2\n")
    assert two["grad"][0]["count"] == 2 and len(two["ops"]) == 1
    assert "grad" not in parse_plan("launch st=0 form=first ty8=1 ty4=0 grid=1 prec=f32 f=3 img=u8 out=f32 ch=3\n")


def _weight_grad(xin, dy, ks):
    """sum over pixels of dy[p] (x) x[p + tap] with zero padding, [O][KH][KW][I]"""
    pad = ks // 2
    H, W = xin.shape[2:]
    xp = np.pad(xin, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    out = np.empty((dy.shape[1], ks, ks, xin.shape[1]))
    for kh in range(ks):
        for kw in range(ks):
            out[:, kh, kw, :] = np.einsum("noyx,niyx->oi", dy, xp[:, :, kh:kh + H, kw:kw + W])
    return out


def test_pixel_terms_add_up_to_the_weight_gradient():
    """the retained nodes are the ones the names say: every convolution's weight gradient is the sum over pixels of dy[p] (x) x[p + tap],
    and pixel_term is one pixel's share of that sum (at an image seam, a corner and an inner pixel)"""
    c = gs.CASES["B"]
    H, W = c["H"], c["W"]
    _, g, kept = gs.restate("B", "synthetic", False, (246,), nodes=True)
    for name in gs.CONV_ORDER:
        xin, dy = kept[name]
        ks = 5 if name in FIVES else 3
        want = seg(g, c["f"], name)
        assert np.linalg.norm(_weight_grad(xin, dy, ks).ravel() - want) <= 1e-12 * np.linalg.norm(want), name
        for p in (246, 247, 0, 300, 740):
            one = np.zeros_like(dy)
            img, r = divmod(p, H * W)
            one[img, :, r // W, r % W] = dy[img, :, r // W, r % W]
            assert np.allclose(gs.pixel_term(kept, name, p, H, W), _weight_grad(xin, one, ks), rtol=1e-13, atol=0), (name, p)
    for conv, bias in BIAS_OF.items():
        assert np.allclose(kept[conv][1].sum(axis=(0, 2, 3)), seg(g, c["f"], bias), rtol=1e-12, atol=0)
    assert np.allclose(kept["conv10"][1].sum(axis=(0, 2, 3)), seg(g, c["f"], "expand_bias"), rtol=1e-12, atol=0)


@pytest.mark.parametrize("row", [r for r in gs.ROWS if not r[2]], ids=gs.row_id)
def test_one_seam_pixel_is_a_hundred_bars(row):
    case, weights, linear, px = row
    c = gs.CASES[case]
    f, H, W = c["f"], c["H"], c["W"]
    err, g, kept = gs.restate(case, weights, linear, gs.pixels(row), nodes=True)
    want_err = gs.AMPLITUDE ** 2 * 3 * f * f * len(px)
    assert abs(err - want_err) <= 1e-5 * want_err   # A^2 3 f^2 per impulse, minus rounding
    ref_err, ref_g = gs.reference(case, weights, linear, gs.pixels(row))
    assert ref_err == err and np.array_equal(ref_g, g)   # the tapped pass is the restatement itself
    for p, tags in px:
        img, r = divmod(p, H * W)
        y, x = divmod(r, W)
        if any(t.startswith("wgrad:chunk") for t in tags):
            for name in gs.CONV_ORDER:   # the term dy[p] (x) x[p + tap] the weight-gradient loop would lose or double
                moved = np.linalg.norm(gs.pixel_term(kept, name, p, H, W))
                assert moved >= MARGIN * gs.norm_bar(seg(g, f, name)), (p, name, moved, gs.norm_bar(seg(g, f, name)))
        if any(t.startswith("colsum:chunk") for t in tags):
            moved = np.linalg.norm(kept["conv10"][1][img, :, y, x])   # d_e[p]
            assert moved >= MARGIN * gs.norm_bar(seg(g, f, "expand_bias")), (p, moved)
        if any(t.startswith("conv:") for t in tags):   # d_z[p] in a workgroup's (wave's) bias partial
            for conv, bias in BIAS_OF.items():
                moved = np.linalg.norm(kept[conv][1][img, :, y, x])
                assert moved >= MARGIN * gs.norm_bar(seg(g, f, bias)), (p, bias, moved)
        if any(t.startswith("image:") for t in tags):   # the neighbouring image's row under a 5x5 tap
            ratio = {name: np.linalg.norm(gs.pixel_term(kept, name, p, H, W, wrap=True)) / gs.norm_bar(seg(g, f, name)) for name in FIVES}
            assert max(ratio.values()) >= MARGIN, (p, ratio)


@pytest.mark.parametrize("case,weights", [("A", "synthetic"), ("A", "imagenet"), ("B", "synthetic"), ("C", "synthetic"), ("D", "synthetic")])
def test_the_restatement_without_an_impulse_is_far_below_the_bar(case, weights):
    f = gs.CASES[case]["f"]
    err0, g0 = gs.reference(case, weights, False, ())
    worst = 0.0
    for row in gs.ROWS:
        if row[0] != case or row[1] != weights or row[2]:
            continue
        _, g = gs.reference(case, weights, False, gs.pixels(row))
        for name in grad_ref.segments(f):
            ratio = np.linalg.norm(seg(g0, f, name)) / gs.norm_bar(seg(g, f, name))
            worst = max(worst, ratio)
            assert ratio <= RESIDUAL, (gs.row_id(row), name, ratio)
    print(f"case {case} ({weights}): impulse-free restatement gradient <= {worst:.2e} of the bar, err {err0:.3e}")
