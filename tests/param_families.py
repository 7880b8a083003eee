"""Seeded parameter sets of sr_net(factor) from families other than the bundled one, and the images and gradient cases the tests run
them on.  Every oracle-parity test used to feed the kernels one statistical family: a bundled .rsr file or `bundled_scale` below (iid
Gaussian conv weights of std 0.03, small biases, betas in [-0.5, 1.5]).  Training makes and consumes others (sr_init_params,
sr_set_params, the validation pass on the current parameters), and three places in the library depend on the scale of the parameters:
the |w| < 2^-14 branch of the host's weight split (sr_api.cpp split_half_host), the subnormal hi halves of small activations in the
split-half mode (sr_kernels.hip split_half2), and the f32 error of the Winograd F(2,3) rows, which depends on the weights.

  bundled_scale  what the suite has always used at factors 2 and 4 (the one generator; three test modules import it from here)
  init           rusty_sr_amd.init_params: conv1..conv10 at std 0.005-0.008, every bias 0, every beta exactly 0 or 1
  early          init after 10 Adam steps (the reference's constants) of the f64 restatement's gradient: correlated, non-Gaussian
  wide           magnitudes spread over 2^14 inside every kernel row and Winograd triple; betas in [-2, 3]
  tiny           conv1..conv10 and every bias 1e-3 of the bundled scale: three quarters of the weights below 2^-14
  dim            conv0 and f_bias 1e-3 of the bundled scale: most of node f below 2^-14, the later nodes at normal size

No GPU here and no fixtures: tests/test_param_families_cpu.py proves on the oracle alone that each family is what it claims to be and
that the reference is well conditioned on it; tests/test_gpu_param_families.py holds the kernels to the oracle on them."""
import os

import numpy as np

import grad_ref
import oracle
from conftest import ROOT, synth_u8

FAMILIES = ("init", "early", "wide", "tiny", "dim")
FACTORS = (2, 3, 4)
IMAGES = ("synth", "noise")
SMALL = 2.0 ** -14          # the smallest normal half: below it split_half_host puts the whole weight into lo
CONVS = ("conv0",) + tuple(f"conv{k}" for k in (1, 2, 3, 5, 6, 7, 8, 9, 10))
LATER_CONVS = CONVS[1:]
BIASES = ("f_bias", "expand_bias", "l1_bias", "l2_bias", "l3_bias")
BETAS = ("f_activ", "l1_activ", "l2_activ", "l3_activ")
ADAM = {"lr": 2e-3, "beta1": 0.95, "beta2": 0.995, "eps": 1e-7, "l2": 1e-6}   # the reference's training constants (main.rs:199-205)
EARLY_STEPS = 10


def seed_of(factor):
    """the seed the tests use at this factor"""
    return 300 + factor


def bundled_scale(factor, seed):
    """No 2x / 4x weights ship with the reference: seeded synthetic parameters with the bundled weights' scales (conv std from
    imagenet.rsr, small biases, BeLU betas in [-0.5, 1.5])."""
    S = grad_ref.segments(factor)
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(grad_ref.num_params(factor)) * 0.03).astype(np.float32)
    b0, a0 = S["f_bias"][0], S["l1_activ"][0]          # f_bias .. l3_bias, f_activ among them; then l1..l3 activ
    p[b0:a0] = (rng.standard_normal(a0 - b0) * 0.05).astype(np.float32)
    fa = S["f_activ"]
    p[fa[0]:fa[0] + fa[1]] = rng.uniform(-0.5, 1.5, fa[1]).astype(np.float32)
    p[a0:a0 + 96] = rng.uniform(-0.5, 1.5, 96).astype(np.float32)
    return p


def _seg(p, factor, name):
    off, n, _ = grad_ref.segments(factor)[name]
    return p[off:off + n]


def _imagenet():
    with open(os.path.join(ROOT, "rusty_sr_amd", "res", "imagenet.rsr"), "rb") as f:
        return oracle.rsr_decode(f.read())


def _init(factor, seed):
    import rusty_sr_amd as r
    return r.init_params(factor, seed)


_EARLY = {}


def early_batch(factor, seed):
    return synth_u8(seed, 2, 12 * factor, 12 * factor)


def _early(factor, seed):
    """init + EARLY_STEPS Adam steps in numpy f64 on the f64 restatement's gradient (MSE of one small batch, the reference's l2)"""
    key = (factor, seed)
    if key not in _EARLY:
        hr = early_batch(factor, seed)
        P = _init(factor, seed).astype(np.float64)
        M, V = np.zeros_like(P), np.zeros_like(P)
        lr, b1, b2, eps = ADAM["lr"], ADAM["beta1"], ADAM["beta2"], ADAM["eps"]
        for t in range(1, EARLY_STEPS + 1):
            _, _, g = grad_ref.backprop(P, hr, factor, False, None, ADAM["l2"])
            M = b1 * M + (1 - b1) * g
            V = b2 * V + (1 - b2) * g * g
            P = P - lr * (M / (1 - b1 ** t)) / (np.sqrt(V / (1 - b2 ** t)) + eps)
        _EARLY[key] = P.astype(np.float32)
    return _EARLY[key].copy()


def _wide(factor, seed):
    p = (_imagenet() if factor == 3 else bundled_scale(factor, seed)).copy()
    rng = np.random.default_rng([seed, 14])
    for name in CONVS:
        off, n, (o, kh, kw, cin) = grad_ref.segments(factor)[name]
        w = p[off:off + n].astype(np.float64).reshape(o, kh, kw, cin)
        w = w * np.exp2(rng.uniform(-12.0, 2.0, (1, kh, kw, cin)))     # one factor per (ky, kx, cin), shared by the output channels
        p[off:off + n] = (w * (0.03 / w.std())).astype(np.float32).ravel()
    for name in BETAS:
        _seg(p, factor, name)[:] = rng.uniform(-2.0, 3.0, 32).astype(np.float32)
    return p


def _scaled(factor, seed, names, s):
    p = bundled_scale(factor, seed)
    for name in names:
        _seg(p, factor, name)[:] *= np.float32(s)
    return p


def family(name, factor, seed):
    """-> the float32 parameters of sr_net(factor) in .rsr order (grad_ref.segments)"""
    if name == "bundled_scale":
        return bundled_scale(factor, seed)
    if name == "init":
        return _init(factor, seed)
    if name == "early":
        return _early(factor, seed)
    if name == "wide":
        return _wide(factor, seed)
    if name == "tiny":
        return _scaled(factor, seed, LATER_CONVS + BIASES, 1e-3)
    if name == "dim":
        return _scaled(factor, seed, ("conv0", "f_bias"), 1e-3)
    raise ValueError(name)


_PARAMS = {}


def weights(name, factor):
    """the one parameter set of (family, factor) that the tests run; "imagenet" (factor 3): the control row"""
    key = (name, factor)
    if key not in _PARAMS:
        if name == "imagenet":
            assert factor == 3
            _PARAMS[key] = _imagenet()
        else:
            _PARAMS[key] = family(name, factor, seed_of(factor))
    return _PARAMS[key]


def share_below(p, factor, names, bound=SMALL):
    v = np.concatenate([_seg(p, factor, n) for n in names])
    return float((np.abs(v) < bound).mean())


# ---- the two images ------------------------------------------------------------------------------------------------------------------
def image(which, factor):
    """"synth": a batch of two with a ragged, odd width (75 = 2 x 32 + 11: the last Winograd output pair is incomplete) and height
    (37 = 4 x 8 + 5): partial tiles on both axes.  "noise": white noise, as in tests/test_gpu_kernel_matrix.py."""
    if which == "synth":
        return synth_u8(200 + factor, 2, 37, 75)
    assert which == "noise"
    return np.random.default_rng(factor).integers(0, 256, (1, 45, 96, 3), dtype=np.uint8)


_TRUTH, _TAPS = {}, {}


def truth(name, factor, which):
    """(f32 oracle output, f64 oracle output) of one (family, factor, image): one oracle run each, shared and left unchanged"""
    key = (name, factor, which)
    if key not in _TRUTH:
        x = oracle.img_to_data(image(which, factor))
        p = weights(name, factor)
        _TRUTH[key] = (oracle.forward_factor(p, x, factor), oracle.forward_factor(p, x, factor, f64=True))
        for a in _TRUTH[key]:
            a.flags.writeable = False
    return _TRUTH[key]


def node_image(which):
    """one image of the factor-3 batch: what sr_read_feature returns is one image's maps"""
    return image(which, 3)[:1]


NODES = ("f", "l1", "l2", "l3")


def taps(name, which):
    """({node: f32}, {node: f64}) of the oracle at factor 3 on node_image(which), and the outputs (f32, f64)"""
    key = (name, which)
    if key not in _TAPS:
        x = oracle.img_to_data(node_image(which))
        p = weights(name, 3)
        o32, t32 = oracle.forward_taps(p, x)
        o64, t64 = oracle.forward_taps(p, x, f64=True)
        _TAPS[key] = (t32, t64, o32, o64)
    return _TAPS[key]


# ---- gradient cases: (family, factor, kind, n, h, w, linear_loss) -----------------------------------------------------------------------
# The gate of tests/test_param_families_cpu.py (the f32 run of the restatement within 1e-5 of the f64 run, per segment) admits a case
# to the GPU table; GATED_OUT names what it refuses, with the measured values in that module.
ALL_GRAD_CASES = [(name, 3, "u8_3", 2, 20, 23, False) for name in FAMILIES] + [
    ("early", 2, "u8_4", 2, 16, 18, True),
    ("wide", 4, "f32", 1, 24, 28, False),
]
GATED_OUT = (("tiny", 3, "u8_3", 2, 20, 23, False), ("dim", 3, "u8_3", 2, 20, 23, False))   # 4.9e-4 and 1.3e-4 against the gate's 1e-5
GRAD_CASES = [c for c in ALL_GRAD_CASES if c not in GATED_OUT]


def grad_case_id(case):
    name, f, kind, n, h, w, linear = case
    return f"{name}-f{f}-{kind}-n{n}-{h}x{w}-{'linear' if linear else 'mse'}"


def grad_case_batch(case):
    """as tests/test_gpu_backprop.py hr_batch makes it"""
    name, f, kind, n, h, w, linear = case
    seed = 1000 + 7 * h + w
    rng = np.random.default_rng(seed)
    if kind == "f32":
        return rng.random((n, h, w, 3), dtype=np.float32)
    px = synth_u8(seed, n, h, w)
    if kind == "u8_4":
        px = np.concatenate([px, rng.integers(0, 256, (n, h, w, 1), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(px)
