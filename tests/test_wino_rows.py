"""The exact mode's stage 1 computes conv1 (5x5, f -> l1) with every kernel row as two Winograd F(2,3) chunks (DESIGN.md 4a, item 4;
sr_kernels.hip half_steps_wino, sr_api.cpp pack_steps_wino).  Restated here on the CPU, on the oracle's own f features: the transform is
the direct convolution, its f32 arithmetic stays far inside the exact mode's bar, and a non-finite pixel reaches exactly its 5x5
receptive field -- the zero tap of the second chunk comes first, so no product ever reads a pixel outside the field of the outputs it
feeds."""
import numpy as np
import pytest

import oracle
from conftest import load_png
import rusty_sr_amd as r

TIGHT = 2e-5  # the exact mode's bar against the f64 oracle (tests/test_gpu_kernel_matrix.py)
CONV1, L1_BIAS, L1_ACTIV = 2683, 2491, 2587  # factor 3 parameter layout (sr_api.cpp ParamLayout)

# positions of a kernel row, in the kernel's order: chunk A (taps 0, 1, 2 on pixels x-2 .. x+1) positions 0-3, then chunk B (a zero tap,
# taps 3, 4 on pixels x .. x+3) positions 1-3.  Accumulator set, the two pixels (columns from x - 2) and whether U is their sum.
ACC = (0, 1, 2, 3, 1, 2, 3)
CA = (0, 1, 2, 1, 3, 4, 3)
CB = (2, 2, 1, 3, 4, 3, 5)
ADD = (False, True, False, False, True, False, False)


def conv1_weights(params):
    return params[CONV1:CONV1 + 25600].reshape(32, 5, 5, 32).astype(np.float64)  # [out][ky][kx][in]


def transformed(w, ky, k):
    """V of position k of kernel row ky, [in][out], in double (the host rounds it once to f32)."""
    g = w[:, ky, :, :]  # [out][kx][in]
    g0, g1, g2 = (g[:, 0], g[:, 1], g[:, 2]) if k < 4 else (np.zeros_like(g[:, 0]), g[:, 3], g[:, 4])
    pos = k if k < 4 else k - 3
    v = (g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2)[pos]
    return v.T


def conv1_direct(f, w):
    H, W, _ = f.shape
    p = np.zeros((H + 4, W + 4, 32))
    p[2:H + 2, 2:W + 2] = f
    y = np.zeros((H, W, 32))
    for ky in range(5):
        for kx in range(5):
            y += p[ky:ky + H, kx:kx + W] @ w[:, ky, kx, :].T
    return y


def conv1_wino(f, w, dtype):
    """Two F(2,3) chunks per kernel row; U, the products, the accumulators and the output transform in `dtype`."""
    H, W, _ = f.shape
    assert W % 2 == 0
    p = np.zeros((H + 4, W + 4, 32), dtype)
    p[2:H + 2, 2:W + 2] = f
    m = [np.zeros((H, W // 2, 32), dtype) for _ in range(4)]
    with np.errstate(invalid="ignore"):
        for ky in range(5):
            rows = p[ky:ky + H]
            d = [rows[:, o:o + W - 1:2] for o in range(6)]  # pixel 2 j + o - 2 of output pair j
            for k in range(7):
                u = d[CA[k]] + d[CB[k]] if ADD[k] else d[CA[k]] - d[CB[k]]
                m[ACC[k]] = m[ACC[k]] + u @ transformed(w, ky, k).astype(dtype)
        y = np.empty((H, W, 32), dtype)
        y[:, 0::2] = (m[0] + m[1]) + m[2]
        y[:, 1::2] = (m[1] - m[2]) - m[3]
    return y


def features(params, x):
    return oracle.forward_taps(params, x[None], f64=True)[1]


def inputs():
    rng = np.random.default_rng(5)
    return {"cartoon_lr": oracle.img_to_data(load_png("cartoon_lr.png"))[:96, :128],
            "white_noise": rng.random((96, 128, 3))}


@pytest.mark.parametrize("weights", r.rsr.BUILTIN)
def test_two_chunk_rows_are_the_direct_convolution(weights):
    params = r.rsr.builtin(weights)
    w = conv1_weights(params)
    beta, bias = params[L1_ACTIV:L1_ACTIV + 32].astype(np.float64), params[L1_BIAS:L1_BIAS + 32].astype(np.float64)
    for name, x in inputs().items():
        t = features(params, x)
        direct = conv1_direct(t["f"], w)
        # the restatement's convention is the oracle's: l1 = BeLU(conv1(f) + b)
        v = direct + bias
        np.testing.assert_allclose(beta * v + np.sqrt(v * v + 1) - 1, t["l1"], rtol=0, atol=1e-9, err_msg=name)
        assert np.abs(conv1_wino(t["f"], w, np.float64) - direct).max() < 1e-12, name
        err = np.abs(conv1_wino(t["f"].astype(np.float32), w, np.float32) - direct).max()
        assert err < TIGHT / 2, (weights, name, err)


def test_a_non_finite_pixel_reaches_exactly_its_receptive_field():
    w = conv1_weights(r.rsr.builtin("imagenet"))
    f = np.random.default_rng(6).random((20, 24, 32))
    for bad in (np.nan, np.inf, -np.inf):
        for (py, px) in ((9, 10), (9, 11), (0, 0), (19, 23)):  # an even and an odd column, the corners
            g = f.copy()
            g[py, px, 7] = bad
            y = conv1_wino(g, w, np.float64)
            field = np.zeros(y.shape[:2], bool)
            field[max(0, py - 2):py + 3, max(0, px - 2):px + 3] = True
            nonfinite = ~np.isfinite(y).all(axis=2)
            np.testing.assert_array_equal(nonfinite, field, err_msg=f"{bad} at {(py, px)}")
