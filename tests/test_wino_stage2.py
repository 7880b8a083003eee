"""The exact mode's stage 2 computes conv2 (5x5 on f) with every kernel row as two Winograd F(2,3) chunks, and conv5 (3x3 on l1) as
direct taps on the same output pairs (sr_kernels.hip half_steps_wino, half_steps_pairs, stage_epilogue_wino).
Restated here on the CPU, as the kernel sums it, on the oracle's own f and l1 features: the f rows go into the four position sets m0-m3,
l1's even-pixel products into m0 and its odd-pixel products into a fifth set m4; y0 = (m0 + m1) + m2, y1 = ((m1 - m2) - m3) + m4.  The
result is the direct stage, its f32 arithmetic stays inside the exact mode's bar (as the direct form's does), and a non-finite value in f or l1 reaches exactly
its 5x5 or 3x3 receptive field."""
import numpy as np
import pytest

import oracle
import rusty_sr_amd as r
from test_wino_rows import ACC, ADD, CA, CB, TIGHT, conv1_direct, inputs, transformed

CONV2, CONV5, L2_BIAS, L2_ACTIV = 28283, 79483, 2523, 2619  # factor 3 parameter layout (sr_api.cpp ParamLayout)


def weights(params):
    w2 = params[CONV2:CONV2 + 25600].reshape(32, 5, 5, 32).astype(np.float64)  # [out][ky][kx][in]
    w5 = params[CONV5:CONV5 + 9216].reshape(32, 3, 3, 32).astype(np.float64)
    return w2, w5


def conv3x3_direct(l1, w):
    H, W, _ = l1.shape
    p = np.zeros((H + 2, W + 2, 32))
    p[1:H + 1, 1:W + 1] = l1
    y = np.zeros((H, W, 32))
    for ky in range(3):
        for kx in range(3):
            y += p[ky:ky + H, kx:kx + W] @ w[:, ky, kx, :].T
    return y


def stage2_wino(f, l1, w2, w5, dtype):
    """conv2 as two F(2,3) chunks per kernel row (V in double, rounded once to `dtype`), conv5 as even / odd direct sums into m0 / m4,
    then the output transform -- every sum in `dtype`, in the kernel's order of sets."""
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
        for ky in range(3):
            for kx in range(3):
                g = w5[:, ky, kx, :].T.astype(dtype)
                m[0] = m[0] + q[ky:ky + H, kx:kx + W - 1:2] @ g       # even pixel 2 j: column 2 j + kx - 1
                m[4] = m[4] + q[ky:ky + H, kx + 1:kx + W:2] @ g       # odd pixel 2 j + 1
        y = np.empty((H, W, 32), dtype)
        y[:, 0::2] = (m[0] + m[1]) + m[2]
        y[:, 1::2] = ((m[1] - m[2]) - m[3]) + m[4]
    return y


def features(params, x):
    return oracle.forward_taps(params, x[None], f64=True)[1]


@pytest.mark.parametrize("wname", r.rsr.BUILTIN)
def test_stage2_as_the_kernel_sums_it_is_the_direct_stage(wname):
    params = r.rsr.builtin(wname)
    w2, w5 = weights(params)
    beta, bias = params[L2_ACTIV:L2_ACTIV + 32].astype(np.float64), params[L2_BIAS:L2_BIAS + 32].astype(np.float64)
    for name, x in inputs().items():
        t = features(params, x)
        direct = conv1_direct(t["f"], w2) + conv3x3_direct(t["l1"], w5)
        # the restatement's convention is the oracle's: l2 = BeLU(conv2(f) + conv5(l1) + b)
        v = direct + bias
        np.testing.assert_allclose(beta * v + np.sqrt(v * v + 1) - 1, t["l2"], rtol=0, atol=1e-9, err_msg=name)
        assert np.abs(stage2_wino(t["f"], t["l1"], w2, w5, np.float64) - direct).max() < 1e-12, name
        err = np.abs(stage2_wino(t["f"].astype(np.float32), t["l1"].astype(np.float32), w2, w5, np.float32) - direct).max()
        # (white noise drives stage 2's sums up to ~63, where f32 rounding alone costs ~1e-5: the direct form in f32 errs as much)
        assert err < TIGHT, (wname, name, err)


def test_a_non_finite_value_reaches_exactly_its_receptive_field():
    w2, w5 = weights(r.rsr.builtin("imagenet"))
    rng = np.random.default_rng(7)
    f, l1 = rng.random((20, 24, 32)), rng.random((20, 24, 32))
    for bad in (np.nan, np.inf, -np.inf):
        for src, R in (("f", 2), ("l1", 1)):
            for (py, px) in ((9, 10), (9, 11), (0, 0), (19, 23)):  # an even and an odd column, the corners
                g, h = f.copy(), l1.copy()
                (g if src == "f" else h)[py, px, 7] = bad
                y = stage2_wino(g, h, w2, w5, np.float64)
                field = np.zeros(y.shape[:2], bool)
                field[max(0, py - R):py + R + 1, max(0, px - R):px + R + 1] = True
                nonfinite = ~np.isfinite(y).all(axis=2)
                np.testing.assert_array_equal(nonfinite, field, err_msg=f"{bad} in {src} at {(py, px)}")
