"""The training graph's passes on the GPU -- pool, forward loss, backward loss, one training step -- on dark, bright, constant and
out-of-range pixels (tests/pixel_classes.py), where the sRGB transfer functions of rusty_sr_amd/csrc/sr_transfer.h, the byte table of
sr_valid.cpp and SrgbToLinear' of sr_grad.hip take the branch that smoothed noise (bytes 37 .. 215) and rng.random never take.  Bars
and restatements are those of test_gpu_validation.py and test_gpu_backprop.py, unchanged; tests/test_pixel_classes_cpu.py shows on
the CPU that every case reaches its branch and is well enough conditioned for its bar."""
import math

import numpy as np
import pytest
import torch

import grad_ref
import pixel_classes as pc
from test_gpu_backprop import assert_grad_close, gpu_pool, validation_err
from test_gpu_validation import POOL_TOL, err_of, oracle_psnr, pool64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor, key="synthetic", precision="f32"):
        k = (factor, key, precision)
        if k not in made:
            made[k] = r.Engine(pc.weights_of(key, factor, params), device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def image(cls, f, k, h, w):
    return pc.make(cls, pc.image_seed(cls, f, h, w), 1, h, w, pc.channels_of(cls, f, k))[0]


# ---- the pool (valid_pool_kernel: srgb_to_linear_fast / the byte table [256, 512), linear_to_srgb_fast) ----------------------------------
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("cls", pc.CLASSES)
def test_pool_matches_restatement(engines, f, cls):
    e = engines(f)
    worst_abs = worst_rel = 0.0
    for k, (h, w) in enumerate(pc.pool_shapes(f)):
        hr = image(cls, f, k, h, w)
        _, n = e.validation_error(hr)
        assert n == 3 * f * (h // f) * f * (w // f)
        lr, _ = e.validation_nodes(h, w)
        want = pool64(hr, f)
        assert lr.shape == want.shape
        err = np.abs(lr.astype(np.float64) - want)
        rel = err / np.maximum(1.0, np.abs(want))
        worst_abs, worst_rel = max(worst_abs, float(err.max())), max(worst_rel, float(rel.max()))
        if cls == "far_f32":      # beyond [-0.5, 1.5] f32 itself keeps the bar only relative to the value (test_pixel_classes_cpu.py)
            assert float(rel.max()) <= POOL_TOL, (h, w, float(rel.max()))
        else:
            assert float(err.max()) <= POOL_TOL, (h, w, float(err.max()))
        if cls == "black":
            assert not lr.any(), (h, w)
        if cls == "white":
            assert float(np.abs(lr - np.float32(1)).max()) <= POOL_TOL, (h, w)
    print(f"pool_error class={cls} f={f} max_abs={worst_abs:.3e} max_rel={worst_rel:.3e}")


# ---- the forward loss (valid_loss_kernel: srgb_to_linear_cr, the byte table [256, 512)) -------------------------------------------------
LOSS_ENGINES = [(2, "synthetic", "f32"), (3, "synthetic", "f32"), (4, "synthetic", "f32"), (3, "imagenet", "f32"), (2, "synthetic", "split_f16")]


@pytest.mark.parametrize("f,key,precision", LOSS_ENGINES, ids=lambda v: str(v))
@pytest.mark.parametrize("cls", pc.CLASSES)
def test_loss_is_exact_to_the_reduction(engines, f, key, precision, cls):
    """The sum of 3 f^2 .. 10^5 squares at rel 1e-12: one value off by an ulp of f32 anywhere moves it by far more.  This is what pins
    srgb_to_linear_cr and the table's SrgbToLinear half as the correctly rounded f32 of the f64 formula on both branches, below 0 and
    above 1.  Crop widths 14, 21 and 90 are not multiples of 4 (the loss kernel's row seams); (f, f) is one LR pixel."""
    e = engines(f, key, precision)
    for k, (h, w) in enumerate(pc.pool_shapes(f)):
        hr = image(cls, f, k, h, w)
        for linear in ((False,) if cls == "far_f32" else (False, True)):
            err, n = e.validation_error(hr, linear_loss=linear)
            _, out = e.validation_nodes(h, w)
            want, m = err_of(out, hr, f, linear)
            assert n == m and math.isfinite(err)
            assert err == pytest.approx(want, rel=1e-12), (h, w, linear, err, want)


@pytest.mark.parametrize("cls,ch", [("dark_u8", 4), ("noise_u8", 3), ("white", 4)])
def test_device_form_scores_the_same_bits(engines, cls, ch):
    """sr_validation_error_rgba8_dev (u8 images only: there is no f32 device form), also from an odd byte address"""
    e = engines(3)
    h, w = 41, 64
    hr = pc.make(cls, 77, 1, h, w, ch)[0]
    for linear in (False, True):
        err, _ = e.validation_error(hr, linear_loss=linear)
        _, out = e.validation_nodes(h, w)
        assert err == pytest.approx(err_of(out, hr, 3, linear)[0], rel=1e-12)
        big = torch.from_numpy(np.concatenate([np.zeros(5, np.uint8), hr.ravel()])).cuda()
        for off in (0, 1, 2, 3):
            view = big[5 - off:5 - off + hr.size]
            view.copy_(torch.from_numpy(hr.ravel()))
            got = e.validation_error_dev(view.view(hr.shape), linear_loss=linear)
            torch.cuda.synchronize()
            assert got.item() == err, (linear, off)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.PSNR_CASES, ids=pc.psnr_case_id)
def test_psnr_end_to_end(engines, params, case):
    import rusty_sr_amd as r
    cls, f, h, w, ch, linear, key = case
    hr = pc.psnr_case_image(case)
    got = r.validation_psnr([engines(f, key)], [hr], linear_loss=linear)
    want = oracle_psnr(("pixel_ranges", cls, key), pc.weights_of(key, f, params), hr, f, linear)
    assert math.isfinite(got) and abs(got - want) <= 0.005, (got, want)


# ---- the backward loss (grad_loss_kernel: srgb_to_linear_cr, srgb_to_linear_deriv, the byte table) -----------------------------------------
@pytest.mark.parametrize("case", pc.GRAD_CASES, ids=pc.grad_case_id)
def test_gradient_matches_restatement(engines, params, case):
    cls, f, n, h, w, ch, linear, key = case
    eng, p = engines(f, key), pc.weights_of(key, f, params)
    hr = pc.grad_case_batch(case)
    err, ne, g = eng.backprop(hr, p, linear_loss=linear)
    assert ne == n * 3 * f * (h // f) * f * (w // f)
    lr, _ = gpu_pool(eng, hr)
    _, ne_ref, want = grad_ref.backprop(p, hr, f, linear, None, 0.0, x=lr.astype(np.float64))
    assert ne_ref == ne
    assert np.isfinite(g).all()
    assert_grad_close(g, want, f, pc.grad_case_id(case))
    val = validation_err(eng, hr, linear)
    assert abs(err - val) <= 1e-6 * val, (err, val)


def test_device_form_of_backprop_is_the_same_bits(engines):
    f = 3
    eng, p = engines(f), pc.synthetic_weights(f)
    hr = pc.make("dark_u8", 31, 2, 10 * f + 1, 11 * f + 2, 4)
    err, _, g = eng.backprop(hr, p, linear_loss=True, l2=1e-6)
    err_d, g_d = eng.backprop_dev(torch.from_numpy(hr).cuda(), torch.from_numpy(p).cuda(), linear_loss=True, l2=1e-6)
    torch.cuda.synchronize()
    assert err_d.item() == err and np.array_equal(g_d.cpu().numpy().view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize("cls,f,ch", [("dark_u8", 2, 3), ("white", 3, 4)])
def test_training_step_is_backprop_then_adam(cls, f, ch):
    """One Trainer.step on such a batch: its err_sum is backprop's, bit for bit; its parameters are those of the device Adam step on
    backprop's gradient, bit for bit, and of the numpy Adam of test_gpu_backprop.test_adam_matches_numpy at that test's bars."""
    import rusty_sr_amd as r
    start = pc.synthetic_weights(f)
    hr = pc.make(cls, 13, 2, 10 * f, 11 * f, ch)
    lr, b1, b2, eps, l2 = 2e-3, 0.95, 0.995, 1e-7, 1e-6
    eng = r.Engine(start, device=0, factor=f)
    try:
        tr = r.Trainer(eng, start, linear_loss=True, l2=l2, lr=lr, beta1=b1, beta2=b2, eps=eps, store_bytes=0)
        try:
            err_t = tr.step(hr)
            got = tr.params()
        finally:
            tr.close()
        err, _, g = eng.backprop(hr, start, linear_loss=True, l2=l2)
        assert err_t == err and np.isfinite(g).all() and g.any()
        pd = torch.from_numpy(start.copy()).cuda()
        md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
        eng.adam_step_dev(pd, md, vd, torch.from_numpy(g).cuda(), 1, lr, b1, b2, eps)
        torch.cuda.synchronize()
        assert np.array_equal(got.view(np.uint32), pd.cpu().numpy().view(np.uint32))
        g64 = g.astype(np.float64)
        M, V = (1 - b1) * g64, (1 - b2) * g64 * g64
        P = start.astype(np.float64) - lr * (M / (1 - b1)) / (np.sqrt(V / (1 - b2)) + eps)
        np.testing.assert_allclose(got, P, rtol=1e-6, atol=1e-5 * lr)
        assert not np.array_equal(got, start)
    finally:
        eng.close()
