"""Backpropagation without a GPU: the f64 restatement of the training graph (tests/grad_ref.py) against the C oracle, the validation
pool's restatement and central finite differences; the backprop ABI in all four places (header, ctypes table, Rust)
and its refusals before the device is touched.  The GPU side: test_gpu_backprop.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_ref
import oracle
from conftest import ROOT
from param_families import bundled_scale as synthetic_params   # (the one generator of bundled-scale weights)

NEW = ["sr_adam_step_dev", "sr_backprop_f32", "sr_backprop_rgba8", "sr_backprop_rgba8_dev"]


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def test_segments_are_the_oracles():
    for f in (2, 3, 4):
        assert grad_ref.num_params(f) == oracle.num_params(f)
    assert {k: v for k, v in grad_ref.segments(3).items()} == oracle.SEGMENTS


@pytest.mark.parametrize("f", [2, 3, 4])
def test_forward_is_the_oracle(f):
    p = synthetic_params(f, 7 + f)
    x = np.random.default_rng(f).random((2, 9, 11, 3))
    want = oracle.forward_factor(p, x, f, f64=True)
    got = grad_ref.forward(torch.from_numpy(p.astype(np.float64)), torch.from_numpy(x), f).numpy()
    assert np.abs(got - want).max() <= 1e-12


def test_pool_is_the_validation_pool():
    """the validation tests' restatement (anchored there on oracle.downsample at factor 3)"""
    rng = np.random.default_rng(3)
    x = rng.random((2, 14, 17, 3), dtype=np.float32)
    np.testing.assert_allclose(grad_ref.pool(grad_ref.hr_values(x[:1]), 3)[0].numpy(), oracle.downsample(x[:1], f64=True)[0],
                               rtol=0, atol=1e-12)
    for f in (2, 3, 4):
        got = grad_ref.pool(grad_ref.hr_values(x), f).numpy()
        lin = lambda v: np.where(v <= grad_ref.THRESH, v / 12.92, ((np.maximum(v, 0.04) + 0.055) / 1.055) ** 2.4)
        srgb = lambda v: np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.maximum(v, 0.0031) ** (1 / 2.4) - 0.055)
        c = x[:, :f * (14 // f), :f * (17 // f)].astype(np.float64)
        want = srgb(lin(c).reshape(2, 14 // f, f, 17 // f, f, 3).mean(axis=(2, 4)))
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("f,linear,l2", [(2, False, 0.0), (3, True, 0.0), (3, False, 0.3), (4, True, 0.05)])
def test_autograd_matches_finite_differences(f, linear, l2):
    p = synthetic_params(f, 20 + f)
    rng = np.random.default_rng(f)
    hr = rng.integers(0, 256, (2, 3 * f + 1, 2 * f + 2, 3), dtype=np.uint8)
    hr64 = grad_ref.hr_values(hr)
    x, target = grad_ref.pool(hr64, f), grad_ref.crop(hr64, f)
    scale = 1.0 / target.numel()
    _, _, g = grad_ref.backprop(p, hr, f, linear, None, l2)
    p64 = torch.from_numpy(p.astype(np.float64))
    pick = np.random.default_rng(100 + f)
    for name, (off, n, _) in grad_ref.segments(f).items():
        for k in pick.choice(n, size=min(n, 3), replace=False):
            i, h = off + int(k), 1e-6
            up, dn = p64.clone(), p64.clone()
            up[i] += h
            dn[i] -= h
            fd = (float(grad_ref.loss(up, x, target, f, linear, scale, l2)[0]) - float(grad_ref.loss(dn, x, target, f, linear, scale, l2)[0])) / (2 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])) + 1e-9, (name, k, fd, g[i])


def test_backprop_symbols_are_declared_exported_and_bound():
    from rusty_sr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", _read(ROOT, "include", "srhip.h"), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    assert [len(_lib.SYMBOLS[n][1]) for n in NEW] == [12, 13, 14, 13]
    import rusty_sr_amd as r
    for m in ("backprop", "backprop_dev", "adam_step_dev"):
        assert callable(getattr(r.Engine, m))
    assert {"step", "params", "save"} <= set(dir(r.Trainer))


def test_backprop_rust_and_integration_declarations_match():
    def decls(text):
        return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"pub fn (sr_backprop\w+|sr_adam_step_dev)\([^)]*\)[^;]*;", text)}
    rs, md = decls(_read(ROOT, "rust_host", "src", "srhip.rs")), decls(_read(ROOT, "INTEGRATION.md"))
    assert sorted(rs) == sorted(md) == NEW
    assert rs == md
    assert "d_grad: *mut f32" in rs["sr_backprop_rgba8_dev"] and "loss_scale: f32" in rs["sr_backprop_f32"]


def _no_device():
    return not torch.cuda.is_available()


def test_backprop_refuses_before_the_gpu():
    """With no HIP device every new entry point says so; with one, a null context is an invalid argument."""
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_NO_DEVICE if _no_device() else _lib.SR_E_INVALID
    err, n = C.c_double(), C.c_size_t()
    p = (C.c_float * 8)()
    g = (C.c_float * 8)()
    buf = (C.c_uint8 * 64)()
    assert L.sr_backprop_rgba8(None, p, 8, buf, 3, 1, 4, 4, 0, 1.0, 0.0, C.byref(err), C.byref(n), g) == want
    assert L.sr_backprop_f32(None, p, 8, p, 1, 4, 4, 0, 1.0, 0.0, C.byref(err), C.byref(n), g) == want
    assert L.sr_backprop_rgba8_dev(None, None, None, 3, 1, 4, 4, 0, 1.0, 0.0, None, None, None) == want
    assert L.sr_adam_step_dev(None, None, None, None, None, 8, 1, 2e-3, 0.95, 0.995, 1e-7, None) == want
    assert list(g) == [0.0] * 8 and err.value == 0.0 and n.value == 0
