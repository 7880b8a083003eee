"""The exact mode's stage 2 computes one 16-channel half of conv5 (3x3 on l1) with every kernel row as ONE Winograd F(2,3) chunk on
the position sets m0-m3 that conv2 already fills, and the other half as direct taps on the output pairs (DESIGN.md 4a, item 4;
sr_kernels.hip half_steps_wino with 3 taps, half_steps_pairs, stage_epilogue_wino).  "wino" = "3" runs both halves as Winograd rows
(a measurement setting).  Restated here on the CPU, as the kernel sums it, on the oracle's own f and l1 features: a Winograd half's
products go into m0-m3, a direct half's even-pixel products into m0 and its odd-pixel products into m4; y0 = (m0 + m1) + m2,
y1 = ((m1 - m2) - m3) + m4.  The result is the direct stage, its f32 arithmetic stays inside the exact mode's bar, and a non-finite
value in l1 reaches exactly its 3x3 receptive field: position 0 (d0 - d2) feeds y0 only, position 3 (d1 - d3) y1 only, and d1, d2 lie
in both fields."""
import numpy as np
import pytest

import rusty_sr_amd as r
from test_wino_rows import ACC, ADD, CA, CB, TIGHT, conv1_direct, inputs, transformed
from test_wino_stage2 import conv3x3_direct, features, weights

HALVES = {"": 1, "3": 2}  # the "wino" setting -> 16-channel halves of conv5 that run as Winograd rows (half 0 first)


def stage2_wino_conv5(f, l1, w2, w5, dtype, nwino):
    """conv2 as two F(2,3) chunks per kernel row; of conv5's two input-channel halves the first `nwino` as one F(2,3) chunk per kernel
    row (positions 0-3 on the pair's pixels 2 j - 1 .. 2 j + 2), the others as even / odd direct sums into m0 / m4 -- V in double and
    rounded once to `dtype`, every sum in `dtype`, in the kernel's order of sets."""
    H, W, _ = f.shape
    assert W % 2 == 0
    p = np.zeros((H + 4, W + 4, 32), dtype)
    p[2:H + 2, 2:W + 2] = f
    q = np.zeros((H + 2, W + 2, 32), dtype)
    q[1:H + 1, 1:W + 1] = l1
    m = [np.zeros((H, W // 2, 32), dtype) for _ in range(5)]
    with np.errstate(invalid="ignore"):
        for ky in range(5):
            rows = p[ky:ky + H]
            d = [rows[:, o:o + W - 1:2] for o in range(6)]  # pixel 2 j + o - 2 of output pair j
            for k in range(7):
                u = d[CA[k]] + d[CB[k]] if ADD[k] else d[CA[k]] - d[CB[k]]
                m[ACC[k]] = m[ACC[k]] + u @ transformed(w2, ky, k).astype(dtype)
        for half in range(2):
            ch = slice(16 * half, 16 * half + 16)
            if half < nwino:
                for ky in range(3):
                    rows = q[ky:ky + H, :, ch]
                    d = [rows[:, o:o + W - 1:2] for o in range(4)]  # pixel 2 j + o - 1 of output pair j
                    for k in range(4):
                        u = d[CA[k]] + d[CB[k]] if ADD[k] else d[CA[k]] - d[CB[k]]
                        m[ACC[k]] = m[ACC[k]] + u @ transformed(w5, ky, k)[ch].astype(dtype)
            else:
                for ky in range(3):
                    for kx in range(3):
                        g = w5[:, ky, kx, ch].T.astype(dtype)
                        m[0] = m[0] + q[ky:ky + H, kx:kx + W - 1:2, ch] @ g   # even pixel 2 j: column 2 j + kx - 1
                        m[4] = m[4] + q[ky:ky + H, kx + 1:kx + W:2, ch] @ g   # odd pixel 2 j + 1
        y = np.empty((H, W, 32), dtype)
        y[:, 0::2] = (m[0] + m[1]) + m[2]
        y[:, 1::2] = ((m[1] - m[2]) - m[3]) + m[4]
    return y


@pytest.mark.parametrize("setting", HALVES, ids=lambda s: s or "default")
@pytest.mark.parametrize("wname", r.rsr.BUILTIN)
def test_stage2_as_the_kernel_sums_it_is_the_direct_stage(wname, setting):
    params = r.rsr.builtin(wname)
    w2, w5 = weights(params)
    for name, x in inputs().items():
        t = features(params, x)
        direct = conv1_direct(t["f"], w2) + conv3x3_direct(t["l1"], w5)
        assert np.abs(stage2_wino_conv5(t["f"], t["l1"], w2, w5, np.float64, HALVES[setting]) - direct).max() < 1e-12, name
        got = stage2_wino_conv5(t["f"].astype(np.float32), t["l1"].astype(np.float32), w2, w5, np.float32, HALVES[setting])
        err = np.abs(got - direct).max()
        print(f"wino={setting!r} {wname} {name}: max |f32 - f64 direct| = {err:.3e}")
        assert err < TIGHT, (setting, wname, name, err)


@pytest.mark.parametrize("setting", HALVES, ids=lambda s: s or "default")
def test_a_non_finite_l1_value_reaches_exactly_its_receptive_field(setting):
    w2, w5 = weights(r.rsr.builtin("imagenet"))
    rng = np.random.default_rng(7)
    f, l1 = rng.random((20, 24, 32)), rng.random((20, 24, 32))
    for bad in (np.nan, np.inf, -np.inf):
        for c in (7, 23):  # a channel of either half
            for (py, px) in ((9, 10), (9, 11), (0, 0), (19, 23)):  # an even and an odd column, the corners
                h = l1.copy()
                h[py, px, c] = bad
                y = stage2_wino_conv5(f, h, w2, w5, np.float64, HALVES[setting])
                field = np.zeros(y.shape[:2], bool)
                field[max(0, py - 1):py + 2, max(0, px - 1):px + 2] = True
                nonfinite = ~np.isfinite(y).all(axis=2)
                np.testing.assert_array_equal(nonfinite, field, err_msg=f"{bad} in l1 channel {c} at {(py, px)}")
