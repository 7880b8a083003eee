"""The training objectives (include/srhip.h sr_set_loss) without a GPU: the f64 restatement tests/loss_ref.py against central finite
differences and against grad_ref, the margins from zero of every table tests/test_gpu_loss.py compares under L1, the two entry points'
refusals before the device is touched, the Python argument checks and the CLI's --loss rules.  The GPU side: test_gpu_loss.py."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

import grad_ref
import loss_ref
from conftest import gpu_available, synth_u8


def _cli(*args):
    from rusty_sr_amd.build import build_host
    return subprocess.run([build_host(), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("kind", ["l1", "charbonnier", "mse"])
@pytest.mark.parametrize("linear", [False, True])
def test_restatement_matches_finite_differences(params, kind, linear):
    """a handful of parameters per segment, on a constructed-margin case: no residual changes sign inside the probe, so |e| is smooth
    there; the bar is test_grad_restatement.py's"""
    f, n, lh, lw = 3, 2, 4, 5
    p = loss_ref.weights(params, f)
    lr, hr = loss_ref.constructed_pair(p, f, n, lh, lw, 11, "f32")
    x, target = loss_ref.lr_values(lr), grad_ref.hr_values(hr)
    scale, l2, eps = 1.0 / target.numel(), 0.05, 1e-2
    _, _, g, margin = loss_ref.backprop(p, hr, f, kind, eps, linear, None, l2, x=x)
    assert margin >= loss_ref.MARGIN_PAIR
    p64 = torch.from_numpy(p.astype(np.float64))
    pick = np.random.default_rng(5)
    for name, (off, cnt, _) in grad_ref.segments(f).items():
        for k in pick.choice(cnt, size=min(cnt, 3), replace=False):
            i, h = off + int(k), 1e-6
            up, dn = p64.clone(), p64.clone()
            up[i] += h
            dn[i] -= h
            fd = (float(loss_ref.loss(up, x, target, f, kind, eps, linear, scale, l2)[0])
                  - float(loss_ref.loss(dn, x, target, f, kind, eps, linear, scale, l2)[0])) / (2 * h)
            assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])) + 1e-9, (name, k, fd, g[i])


@pytest.mark.parametrize("linear", [False, True])
def test_mse_is_grad_ref_exactly(params, linear):
    p = params["imagenet"]
    hr = synth_u8(3, 2, 13, 11)
    e0, n0, g0 = grad_ref.backprop(p, hr, 3, linear, 0.37, 0.02)
    e1, n1, g1, _ = loss_ref.backprop(p, hr, 3, "mse", 1e-3, linear, 0.37, 0.02)
    assert e0 == e1 and n0 == n1 and np.array_equal(g0, g1)


def test_objectives_at_their_special_points():
    e = torch.tensor([-2.0, 0.0, 0.5], dtype=torch.float64, requires_grad=True)
    loss_ref.rho(e, "l1", 0.0).sum().backward()
    assert e.grad.tolist() == [-1.0, 0.0, 1.0]          # the subgradient at 0 is 0
    e.grad = None
    loss_ref.rho(e, "charbonnier", 0.25).sum().backward()
    want = [v / math.sqrt(v * v + 0.0625) for v in (-2.0, 0.0, 0.5)]
    assert np.allclose(e.grad.numpy(), want, rtol=1e-15, atol=0) and float(loss_ref.rho(e.detach(), "charbonnier", 0.25)[1]) == 0.0


def test_constructed_pairs_keep_their_margin(params):
    """every constructed pair test_gpu_loss.py runs under L1: min |e| >= MARGIN_PAIR in the loss's own domain"""
    for f, n, lh, lw in loss_ref.PAIR_CASES:
        p = loss_ref.weights(params, f)
        for target in ("f32", "u8"):
            lr, hr = loss_ref.constructed_pair(p, f, n, lh, lw, loss_ref.pair_seed(lh, lw), target)
            assert hr.shape == (n, f * lh, f * lw, 3) and hr.dtype == (np.float32 if target == "f32" else np.uint8)
            for linear in (False, True):
                m = loss_ref.backprop(p, hr, f, "l1", linear=linear, x=loss_ref.lr_values(lr))[3]
                assert m >= loss_ref.MARGIN_PAIR, (f, n, lh, lw, target, linear, m)


def test_pooled_cases_keep_their_margin(params):
    """the searched seeds of the pooled forms: min |e| >= MARGIN_POOL; and the search finds them again"""
    for f, n, h, w, linear, seed in loss_ref.POOL_CASES:
        p = loss_ref.weights(params, f)
        m = loss_ref.backprop(p, synth_u8(seed, n, h, w), f, "l1", linear=linear)[3]
        assert m >= loss_ref.MARGIN_POOL, (f, n, h, w, linear, seed, m)
        assert loss_ref.find_pool_seed(p, f, n, h, w, linear) == seed


def test_last_pair_case_takes_more_than_one_chunk():
    """(sr_grad.hip layout: a loss workgroup per 256 LR pixels, a weight-gradient chunk per 512, a column-sum chunk per 1024)"""
    f, n, lh, lw = loss_ref.PAIR_CASES[-1]
    assert n * lh * lw > 2 * 256 and -(-n * lh * lw // 512) > 1


def test_null_context_is_refused_before_the_gpu():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_INVALID if gpu_available() else _lib.SR_E_NO_DEVICE
    kind, eps = C.c_int(7), C.c_float(0.5)
    for k in (_lib.SR_LOSS_MSE, _lib.SR_LOSS_L1, _lib.SR_LOSS_CHARBONNIER, 3):
        assert L.sr_set_loss(None, k, 1e-3) == want
    assert L.sr_get_loss(None, C.byref(kind), C.byref(eps)) == want
    assert kind.value == 7 and eps.value == 0.5
    assert (_lib.SR_LOSS_MSE, _lib.SR_LOSS_L1, _lib.SR_LOSS_CHARBONNIER) == (0, 1, 2)
    assert len(_lib.SYMBOLS["sr_set_loss"][1]) == 3 and len(_lib.SYMBOLS["sr_get_loss"][1]) == 3


def test_parse_loss_spec():
    import rusty_sr_amd as r
    assert r.parse_loss_spec("mse") == ("mse", 1e-3) and r.parse_loss_spec("l1") == ("l1", 1e-3)
    assert r.parse_loss_spec("charbonnier") == ("charbonnier", 1e-3)
    assert r.parse_loss_spec("charbonnier:0.01") == ("charbonnier", float(np.float32(0.01)))
    assert r.parse_loss_spec("charbonnier:1") == ("charbonnier", 1.0) and r.parse_loss_spec("charbonnier:.5e-1")[1] == float(np.float32(0.05))
    for bad in ("", "L1", "huber", "mse:0.1", "l1:", "charbonnier:", "charbonnier:0", "charbonnier:-0.1", "charbonnier:1.5", "charbonnier:nan",
                "charbonnier:inf", "charbonnier:1e-60", "charbonnier:0x1p-3", "charbonnier: 0.1", "charbonnier:0.1:2", "charbonnier:1e999"):
        with pytest.raises(ValueError) as e:
            r.parse_loss_spec(bad)
        assert "--loss" in str(e.value), bad


def test_engine_set_loss_checks_its_arguments_before_the_library():
    import rusty_sr_amd as r

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    eng = r.Engine.__new__(r.Engine)   # no context: only the argument checks may run
    eng._L, eng._ctx = Untouchable(), None
    for kind, eps in (("huber", 1e-3), ("L1", 1e-3), (1, 1e-3), ("charbonnier", 0.0), ("charbonnier", -1.0), ("charbonnier", float("nan")),
                      ("charbonnier", float("inf")), ("charbonnier", 1.5), ("charbonnier", 1e-60), ("charbonnier", "x"), ("charbonnier", None)):
        with pytest.raises(ValueError):
            eng.set_loss(kind, eps)
    assert set(r.Engine.LOSSES) == set(loss_ref.KINDS)
    import inspect
    sig = inspect.signature(r.Trainer.__init__).parameters
    assert sig["loss"].default == "mse" and sig["loss_eps"].default == 1e-3


def test_cli_loss_rules(tmp_path):
    """help text; a malformed value, and --loss anywhere but `train`, are exit 2 naming --loss -- before any file or device is looked at"""
    res = _cli("train", "--help")
    assert res.returncode == 0 and "--loss <LOSS>" in res.stdout and "charbonnier[:EPS]" in res.stdout
    out, folder = str(tmp_path / "p.rsr"), str(tmp_path / "missing")
    for bad in ("huber", "L1", "mse:1", "l1:0.1", "charbonnier:", "charbonnier:0", "charbonnier:-1", "charbonnier:1.5", "charbonnier:nan",
                "charbonnier:inf", "charbonnier:1e-60", "charbonnier:0x10", "charbonnier: 1", "charbonnier:0.1:2", "charbonnier:" + "9" * 400, ""):
        res = _cli("train", "--loss", bad, out, folder)
        assert res.returncode == 2 and "'--loss <LOSS>'" in res.stderr and "USAGE" in res.stderr, (bad, res.stderr)
        assert res.stderr.endswith("For more information try --help\n") and not res.stdout
    res = _cli("train", "--loss")
    assert res.returncode == 2 and "'--loss <LOSS>' requires a value" in res.stderr
    # a good value passes the option parser: the refusal is then the folder's
    for good in ("mse", "l1", "charbonnier", "charbonnier:0.01", "charbonnier:1", "charbonnier:5e-4"):
        res = _cli("train", "--loss", good, "-l", "--augment", out, folder)
        assert res.returncode == 2 and "is not a folder" in res.stderr and "--loss" not in res.stderr, (good, res.stderr)
    for argv in (("--loss", "l1", "a.png", "b.png"), ("validate", "--loss", "l1", str(tmp_path)), ("video", "--loss", "l1", "-", "-")):
        res = _cli(*argv)
        assert res.returncode == 2 and "'--loss' can only be used with the 'train' subcommand" in res.stderr, (argv, res.stderr)
    assert not (tmp_path / "p.rsr").exists()
