"""The training objectives of include/srhip.h sr_set_loss restated in torch f64 on tests/grad_ref.py's graph (its forward, pool, s2l and
crop, unchanged), the constructed targets whose residuals stay clear of zero, and the tables tests/test_gpu_loss.py runs --
tests/test_loss_cpu.py checks the restatement against finite differences and asserts the margins on these very tables.

  e    = output - hr, or SrgbToLinear(output) - SrgbToLinear(hr)         (grad_ref.loss's e)
  loss = loss_scale * sum rho(e) + l2 * sum p^2
  rho  = e^2 ("mse") | |e| ("l1": torch's abs, subgradient 0 at 0) | sqrt(e^2 + eps^2) - eps ("charbonnier")

An L1 gradient is discontinuous in e: the sign of ONE residual that an f32 forward pass and this f64 one see on different sides of zero
moves the parameter gradient by 1e-2 and more, a hundred times assert_grad_close's bars.  So a comparison under "l1" may only use
inputs whose f64 residuals keep a margin from zero: MARGIN_PAIR for the constructed targets (any shape, through the pair forms),
MARGIN_POOL for the pooled forms, whose target is also the input and cannot be constructed -- their seeds are searched (find_pool_seed
is the search that found POOL_CASES' seeds)."""
import numpy as np
import torch

import grad_ref
from conftest import synth_u8

from param_families import bundled_scale

KINDS = ("mse", "l1", "charbonnier")


def weights(params, f):
    """the parameters the tables below were made for: imagenet.rsr at factor 3, bundled-scale synthetic ones at 2 and 4"""
    return params["imagenet"] if f == 3 else bundled_scale(f, 100 + f)


MARGIN_PAIR = 1e-3   # min |e| of a constructed pair, in the loss's own domain
MARGIN_POOL = 1e-4   # ... of a searched pooled case: the project's f32 forward parity bar, ~500 x the f32-vs-f64 forward difference


def rho(e, kind, eps):
    if kind == "mse":
        return e * e
    if kind == "l1":
        return e.abs()
    if kind == "charbonnier":
        return torch.sqrt(e * e + eps * eps) - eps
    raise ValueError(kind)


def residual(p, x, hr64, f, linear=False):
    out = grad_ref.forward(p, x, f)
    return (grad_ref.s2l(out) - grad_ref.s2l(hr64)) if linear else (out - hr64)


def loss(p, x, hr64, f, kind="mse", eps=1e-3, linear=False, loss_scale=1.0, l2=0.0):
    """(scaled loss, err_sum = sum e^2 under every kind) for LR input x (n, H, W, 3) and the HR crop hr64 (n, fH, fW, 3), both f64."""
    e = residual(p, x, hr64, f, linear)
    return loss_scale * rho(e, kind, eps).sum() + l2 * (p * p).sum(), (e * e).sum()


def _as64(a):
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64)
    return a[None] if a.dim() == 3 else a


def backprop(params, hr, f, kind="mse", eps=1e-3, linear=False, loss_scale=None, l2=0.0, x=None):
    """grad_ref.backprop under an objective: hr (n, h, w, 3|4) u8 or (n, h, w, 3) f32; x: the network's input (default: grad_ref's f64
    pool of hr).  -> (err_sum, n_elems, grad f64 numpy, min |e|)."""
    hr64 = grad_ref.hr_values(hr)
    if hr64.dim() == 3:
        hr64 = hr64[None]
    x = grad_ref.pool(hr64, f) if x is None else _as64(x)
    target = grad_ref.crop(hr64, f)
    if loss_scale is None:
        loss_scale = 1.0 / target.numel()
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    e = residual(p, x, target, f, linear)
    total = loss_scale * rho(e, kind, eps).sum() + l2 * (p * p).sum()
    total.backward()
    return float((e * e).sum().detach()), target.numel(), p.grad.numpy(), float(e.detach().abs().min())


def lr_values(lr):
    """What the network reads of a paired call's LR batch: byte / 255 in f32 (alpha dropped) or the f32 image; (n, H, W, 3) f64."""
    return _as64(grad_ref.hr_values(lr).numpy())


def constructed_pair(params, f, n, lh, lw, seed, target="f32"):
    """An LR batch and an HR target a distance away from the f64 output on it: LR = synth_u8 (u8, or byte / 255 in f32 for an f32 target);
    f32 target = float32(out64 + d), |d| uniform in [0.02, 0.25] with a seeded sign; u8 target = clip(round(255 out64) + k), |k| in
    6..40, the sign flipped wherever the sum would leave 0..255.  -> (lr, hr) as the pair calls take them."""
    rng = np.random.default_rng(seed)
    lr8 = synth_u8(seed, n, lh, lw)
    lr = lr8 if target == "u8" else lr8.astype(np.float32) / np.float32(255)
    with torch.no_grad():
        out64 = grad_ref.forward(torch.from_numpy(np.asarray(params, dtype=np.float64)), lr_values(lr), f).numpy()
    sign = np.where(rng.integers(0, 2, out64.shape) == 1, 1.0, -1.0)
    if target == "f32":
        return lr, (out64 + sign * rng.uniform(0.02, 0.25, out64.shape)).astype(np.float32)
    base = np.rint(255.0 * out64)
    k = sign * rng.integers(6, 41, out64.shape)
    k = np.where((base + k < 0) | (base + k > 255), -k, k)
    return lr, np.clip(base + k, 0, 255).astype(np.uint8)


def find_pool_seed(params, f, n, h, w, linear, seeds=range(64), margin=MARGIN_POOL):
    """The first seed whose synth_u8(seed, n, h, w), pooled, leaves min |e| >= margin (None: no seed of `seeds` does)."""
    for s in seeds:
        if backprop(params, synth_u8(s, n, h, w), f, "l1", linear=linear)[3] >= margin:
            return s
    return None


# ---- the tables of tests/test_gpu_loss.py
PAIR_CASES = [  # (factor, n, LR h, LR w)
    (3, 1, 1, 1),
    (3, 4, 5, 7),
    (2, 2, 8, 9),
    (4, 1, 3, 4),
    (3, 2, 20, 21),   # 840 LR pixels: 4 loss workgroups (256 pixels each) and 2 weight-gradient chunks (512 pixels each)
]
# (factor, n, h, w, linear, seed): searched with find_pool_seed over seeds 0..63 on the weights test_gpu_loss.py uses (imagenet.rsr)
POOL_CASES = [
    (3, 1, 3, 3, False, 0),     # an LR image of 1 x 1
    (3, 1, 12, 15, False, 5),
    (3, 1, 14, 16, True, 2),    # sizes not divisible by f
    (3, 2, 10, 9, True, 2),
    (2, 2, 6, 9, False, 1),
    (4, 1, 9, 8, True, 0),
]


def pair_seed(lh, lw):
    return 100 + lh * lw
