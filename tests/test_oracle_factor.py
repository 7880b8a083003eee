"""An independent float64 anchor for sr_net(factor) at factors other than 3.

No weights for factor 2 or 4 ship with the reference, so what the graph computes there is the C oracle's reading of network.rs
(sr_oracle.c, forward_factor); the HIP engine is tested against that reading.  Here the reading itself is checked against a short
torch-float64 restatement that shares no code with the oracle: parameter offsets derived from the factor (only the expand node's
3 f^2 channels depend on it), Expand as an index shuffle with channel (dy f + dx) 3 + c, LinearInterp as F.interpolate (half-pixel
centres, edges replicated)."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, ROOT, synth_u8

torch = pytest.importorskip("torch")
F = torch.nn.functional

# op insertion order of network.rs:33-72 with the factor-3 sizes; 27 (= 3 f^2 at f = 3) is the expand node's channel count
LAYOUT = [("conv0", (32, 5, 5, 3)), ("f_bias", (32,)), ("f_activ", (32,)), ("expand_bias", (27,)), ("l1_bias", (32,)),
          ("l2_bias", (32,)), ("l3_bias", (32,)), ("l1_activ", (32,)), ("l2_activ", (32,)), ("l3_activ", (32,)),
          ("conv1", (32, 5, 5, 32)), ("conv2", (32, 5, 5, 32)), ("conv3", (32, 5, 5, 32)), ("conv5", (32, 3, 3, 32)),
          ("conv6", (32, 3, 3, 32)), ("conv7", (27, 3, 3, 32)), ("conv8", (32, 3, 3, 32)), ("conv9", (27, 3, 3, 32)),
          ("conv10", (27, 3, 3, 32))]


def split_params(p, f):
    out, pos = {}, 0
    for key, shape in LAYOUT:
        shape = tuple(3 * f * f if d == 27 else d for d in shape)
        cnt = int(np.prod(shape))
        out[key] = torch.from_numpy(np.asarray(p[pos:pos + cnt], dtype=np.float64).reshape(shape))
        pos += cnt
    assert pos == len(p), (pos, len(p))
    return out


def conv(x, w):  # w stored [O][KH][KW][I]; cross-correlation, zero "same" padding
    return F.conv2d(x, w.permute(0, 3, 1, 2).contiguous(), padding=w.shape[1] // 2)


def belu(x, bias, beta):
    x = x + bias.view(1, -1, 1, 1)
    return beta.view(1, -1, 1, 1) * x + torch.sqrt(x * x + 1.0) - 1.0


def sr_net(p, x, f):
    """x (n,H,W,3) float -> (n,fH,fW,3) float64."""
    p = split_params(p, f)
    x = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2).contiguous()
    n, _, H, W = x.shape
    fm = belu(conv(x, p["conv0"]), p["f_bias"], p["f_activ"])
    l1 = belu(conv(fm, p["conv1"]), p["l1_bias"], p["l1_activ"])
    l2 = belu(conv(fm, p["conv2"]) + conv(l1, p["conv5"]), p["l2_bias"], p["l2_activ"])
    l3 = belu(conv(fm, p["conv3"]) + conv(l1, p["conv6"]) + conv(l2, p["conv8"]), p["l3_bias"], p["l3_activ"])
    e = conv(l1, p["conv7"]) + conv(l2, p["conv9"]) + conv(l3, p["conv10"]) + p["expand_bias"].view(1, -1, 1, 1)
    out = F.interpolate(x, scale_factor=f, mode="bilinear", align_corners=False)
    # Expand: out[f y + dy][f x + dx][c] += e[y][x][(dy f + dx) 3 + c]
    out = out + e.view(n, f, f, 3, H, W).permute(0, 3, 4, 1, 5, 2).reshape(n, 3, f * H, f * W)
    return out.permute(0, 2, 3, 1).contiguous().numpy()


def _synthetic(f, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(oracle.num_params(f)) * 0.05).astype(np.float32)
    e = 3 * f * f
    p[2432:2464] = rng.uniform(-0.5, 1.5, 32).astype(np.float32)            # f_activ
    p[2464 + e + 96:2464 + e + 192] = rng.uniform(-0.5, 1.5, 96).astype(np.float32)  # l1..l3 activ
    return p


def test_layout_matches_the_oracle_count():
    for f in (2, 3, 4):
        assert sum(int(np.prod(tuple(3 * f * f if d == 27 else d for d in s))) for _, s in LAYOUT) == oracle.num_params(f)


@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (1, 2, 3), (1, 5, 7), (1, 9, 33), (2, 6, 11)])
def test_forward_factor_f64_against_torch(params, f, n, h, w):
    p = params["imagenet"] if f == 3 else _synthetic(f, 40 + f)
    x = oracle.img_to_data(synth_u8(7 * h + w, n, h, w)).astype(np.float64)
    want = sr_net(p, x, f)
    got = oracle.forward_factor(p, x, f, f64=True)
    assert got.shape == want.shape == (n, f * h, f * w, 3)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("f", [2, 4])
def test_white_noise_and_out_of_range_inputs(f):
    """Pre-activations far out (white noise, inputs outside [0, 1]): the same bar."""
    p = _synthetic(f, 50 + f)
    rng = np.random.default_rng(f)
    x = rng.random((1, 12, 17, 3)) * 3 - 1
    want = sr_net(p, x, f)
    assert np.abs(oracle.forward_factor(p, x, f, f64=True) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_restatement_reproduces_the_committed_factor3_vectors():
    """At f = 3 the restatement meets the committed torch-float64 node vectors (tests/golden/make_vectors.py), stored as f32."""
    v = np.load(os.path.join(GOLDEN, "vectors_torch_f64.npz"))
    for case in ("crop", "border", "one", "twothree"):
        with open(os.path.join(ROOT, "rusty_sr_amd", "res", str(v[f"{case}.weights"]) + ".rsr"), "rb") as fh:
            p = oracle.rsr_decode(fh.read())
        px = v[f"{case}.px"]
        got = sr_net(p, (px.astype(np.float64) / 255.0)[None], 3)[0]
        want = v[f"{case}.out"]
        assert got.shape == want.shape
        # (f32 rounding of the stored vectors: half an ulp of values below 2)
        assert np.abs(got - want.astype(np.float64)).max() <= 2.0 ** -24 * max(1.0, np.abs(want).max()), case
        assert np.abs(oracle.forward_factor(p, px.astype(np.float64)[None] / 255.0, 3, f64=True)[0] - got).max() <= 1e-12, case
