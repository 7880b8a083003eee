"""Backpropagation on the GPU (include/srhip.h sr_backprop_*, sr_adam_step_dev) against the f64 autograd restatement of the training
graph (tests/grad_ref.py), the validation pass (err_sum) and a numpy restatement of Adam."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import grad_ref
from conftest import load_png, synth_u8
from test_grad_restatement import synthetic_params

pytestmark = pytest.mark.gpu


def hr_batch(kind, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "f32":
        return rng.random((n, h, w, 3), dtype=np.float32)
    px = synth_u8(seed, n, h, w)
    if kind == "u8_4":
        px = np.concatenate([px, rng.integers(0, 256, (n, h, w, 1), dtype=np.uint8)], axis=-1)
    return np.ascontiguousarray(px)


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision="f32"):
        k = (factor, precision)
        if k not in made:
            made[k] = r.Engine(weights(params, factor), device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def weights(params, f):
    return params["imagenet"] if f == 3 else synthetic_params(f, 100 + f)


def gpu_pool(eng, hr):
    """the GPU's own pooled input of each image (the validation pass's pool, which test_gpu_validation.py holds to its restatement)
    and the sum of the per-image validation errors"""
    lrs, err = [], 0.0
    for img in hr:
        e, _ = eng.validation_error(img, False)
        lrs.append(eng.validation_nodes(img.shape[0], img.shape[1])[0])
        err += e
    return np.stack(lrs), err


def validation_err(eng, hr, linear):
    return math.fsum(eng.validation_error(img, linear)[0] for img in hr)


def assert_grad_close(g, want, f, what=""):
    g, want = g.astype(np.float64), want.astype(np.float64)
    for name, (off, n, _) in grad_ref.segments(f).items():
        d, w = g[off:off + n] - want[off:off + n], want[off:off + n]
        floor = 1e-7 * np.abs(want).max()
        assert np.linalg.norm(d) <= 1e-4 * np.linalg.norm(w) + floor, (what, name, np.linalg.norm(d), np.linalg.norm(w))
        assert np.abs(d).max() <= 1e-3 * np.abs(w).max() + floor, (what, name, np.abs(d).max(), np.abs(w).max())


CASES = [  # (factor, kind, n, h, w, linear_loss)
    (3, "u8_3", 1, 3, 3, False),        # an LR image of 1 x 1
    (3, "u8_4", 4, 20, 23, True),       # sizes not divisible by f
    (3, "f32", 1, 17, 16, False),
    (3, "u8_3", 2, 30, 33, False),
    (2, "u8_3", 4, 16, 18, True),
    (2, "f32", 1, 2, 5, False),
    (2, "u8_4", 1, 21, 20, False),
    (4, "u8_4", 1, 4, 4, True),         # LR 1 x 1
    (4, "u8_3", 4, 33, 30, False),
    (4, "f32", 2, 24, 28, True),
    (3, "u8_3", 4, 192, 192, False),    # the reference's training step (main.rs:181-205: batch 4, 192 px crops)
    (3, "u8_4", 2, 384, 384, True),
]


@pytest.mark.parametrize("f,kind,n,h,w,linear", CASES)
def test_gradient_matches_restatement(engines, params, f, kind, n, h, w, linear):
    eng = engines(f)
    p = weights(params, f)
    hr = hr_batch(kind, n, h, w, 1000 + 7 * h + w)
    err, ne, g = eng.backprop(hr, p, linear_loss=linear)
    assert ne == n * 3 * f * (h // f) * f * (w // f)
    lr, _ = gpu_pool(eng, hr)
    _, ne_ref, want = grad_ref.backprop(p, hr, f, linear, None, 0.0, x=lr.astype(np.float64))
    assert ne_ref == ne
    assert np.isfinite(g).all()
    assert_grad_close(g, want, f, (f, kind, n, h, w, linear))
    val = validation_err(eng, hr, linear)
    assert abs(err - val) <= 1e-6 * val, (err, val)


def test_scale_and_l2_are_linear(engines, params):
    eng, p = engines(3), params["imagenet"]
    hr = hr_batch("u8_3", 2, 24, 27, 5)
    _, _, g1 = eng.backprop(hr, p, loss_scale=1.0, l2=0.0)
    s, lam = 0.37, 0.021
    _, _, g = eng.backprop(hr, p, loss_scale=s, l2=lam)
    want = s * g1.astype(np.float64) + 2 * lam * p.astype(np.float64)
    assert np.linalg.norm(g - want) <= 1e-6 * np.linalg.norm(want)


def test_batch_is_the_sum_of_its_images(engines, params):
    eng, p = engines(2), weights(params, 2)
    hr = hr_batch("u8_4", 3, 14, 17, 9)
    err, ne, g = eng.backprop(hr, p, loss_scale=1.0)
    parts = [eng.backprop(hr[i:i + 1], p, loss_scale=1.0) for i in range(3)]
    assert ne == sum(q[1] for q in parts)
    assert abs(err - math.fsum(q[0] for q in parts)) <= 1e-9 * err
    want = sum(q[2].astype(np.float64) for q in parts)
    assert np.linalg.norm(g - want) <= 1e-5 * np.linalg.norm(want)


def test_bits_are_reproducible(engines, params):
    import rusty_sr_amd as r
    eng, p = engines(3), params["imagenet"]
    hr = hr_batch("u8_4", 2, 40, 44, 11)
    a = eng.backprop(hr, p, linear_loss=True, l2=1e-6)
    b = eng.backprop(hr, p, linear_loss=True, l2=1e-6)
    assert a[0] == b[0] and np.array_equal(a[2], b[2])
    other = r.Engine(p, device=0, factor=3)
    try:
        c = other.backprop(hr, p, linear_loss=True, l2=1e-6)
    finally:
        other.close()
    assert a[0] == c[0] and np.array_equal(a[2], c[2])
    split = engines(3, "split_f16")
    d = split.backprop(hr, p, linear_loss=True, l2=1e-6)
    assert a[0] == d[0] and np.array_equal(a[2], d[2])
    # the device form: the same bits
    hr_d = torch.from_numpy(hr).cuda()
    p_d = torch.from_numpy(p).cuda()
    err_d, g_d = eng.backprop_dev(hr_d, p_d, linear_loss=True, l2=1e-6)
    torch.cuda.synchronize()
    assert err_d.item() == a[0] and np.array_equal(g_d.cpu().numpy(), a[2])


def test_gradient_is_of_the_params_passed(engines, params):
    eng = engines(3)  # inference weights: imagenet
    p = synthetic_params(3, 77)
    hr = hr_batch("u8_3", 1, 12, 15, 3)
    err, _, g = eng.backprop(hr, p)
    lr, _ = gpu_pool(eng, hr)
    e_ref, _, want = grad_ref.backprop(p, hr, 3, x=lr.astype(np.float64))
    assert_grad_close(g, want, 3)
    assert abs(err - e_ref) <= 1e-5 * e_ref


def test_refusals_leave_outputs_untouched(engines, params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    eng, p = engines(3), params["imagenet"]
    L = _lib.lib()
    fp = C.POINTER(C.c_float)
    g = np.full(p.size, 7.0, dtype=np.float32)
    err, ne = C.c_double(5.0), C.c_size_t(3)
    hr = hr_batch("u8_3", 1, 9, 9, 1)
    u8 = hr.ctypes.data_as(C.POINTER(C.c_uint8))
    call = lambda np_, ch, h, w: L.sr_backprop_rgba8(eng._ctx, p.ctypes.data_as(fp), np_, u8, ch, 1, h, w, 0, 1.0, 0.0, C.byref(err),
                                                     C.byref(ne), g.ctypes.data_as(fp))
    assert call(p.size - 1, 3, 9, 9) == _lib.SR_E_PARAM_COUNT
    assert call(p.size, 3, 2, 9) == _lib.SR_E_INVALID   # h < f
    assert call(p.size, 3, 9, 2) == _lib.SR_E_INVALID
    assert call(p.size, 2, 9, 9) == _lib.SR_E_INVALID
    assert (g == 7.0).all() and err.value == 5.0 and ne.value == 3
    # device form: misaligned pointers refused before any launch
    hr_d = torch.from_numpy(hr).cuda()
    p_d = torch.from_numpy(np.concatenate([[0], p]).astype(np.float32)).cuda()
    g_d = torch.full((p.size + 1,), 7.0, device="cuda")
    e_d = torch.full((2,), 5.0, dtype=torch.float64, device="cuda")
    vp = C.c_void_p
    odd = lambda t, b: vp(t.data_ptr() + b)
    dev = lambda pp, ee, gg: L.sr_backprop_rgba8_dev(eng._ctx, pp, vp(hr_d.data_ptr()), 3, 1, 9, 9, 0, 1.0, 0.0, ee, gg, None)
    assert dev(odd(p_d, 2), vp(e_d.data_ptr()), vp(g_d.data_ptr())) == _lib.SR_E_INVALID
    assert dev(vp(p_d.data_ptr()), odd(e_d, 2), vp(g_d.data_ptr())) == _lib.SR_E_INVALID
    assert dev(vp(p_d.data_ptr()), vp(e_d.data_ptr()), odd(g_d, 1)) == _lib.SR_E_INVALID
    torch.cuda.synchronize()
    assert (g_d.cpu() == 7.0).all() and (e_d.cpu() == 5.0).all()
    bil = r.Engine((), device=0, graph="bilinear")
    try:
        assert L.sr_backprop_rgba8(bil._ctx, p.ctypes.data_as(fp), p.size, u8, 3, 1, 9, 9, 0, 1.0, 0.0, C.byref(err), C.byref(ne),
                                   g.ctypes.data_as(fp)) == _lib.SR_E_INVALID
    finally:
        bil.close()
    assert (g == 7.0).all()
    # the context is still usable
    e2, _, g2 = eng.backprop(hr, p)
    assert np.isfinite(g2).all() and e2 > 0


def test_full_hd_image(engines, params):
    eng, p = engines(3), params["imagenet"]
    hr = hr_batch("u8_3", 1, 1080, 1920, 21)
    a = eng.backprop(hr, p, linear_loss=True)
    b = eng.backprop(hr, p, linear_loss=True)
    assert np.isfinite(a[2]).all() and np.array_equal(a[2], b[2]) and a[0] == b[0]
    val = eng.validation_error(hr[0], True)[0]
    assert abs(a[0] - val) <= 1e-6 * val


def test_adam_matches_numpy(engines):
    eng = engines(3)
    rng = np.random.default_rng(4)
    n = 5000
    p = rng.standard_normal(n).astype(np.float32)
    grads = [rng.standard_normal(n).astype(np.float32) * s for s in (1.0, 0.01, 3.0)]
    pd, md, vd = torch.from_numpy(p.copy()).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    P, M, V = p.astype(np.float64), np.zeros(n), np.zeros(n)
    lr, b1, b2, eps = 2e-3, 0.95, 0.995, 1e-7
    for t, g in enumerate(grads, 1):
        eng.adam_step_dev(pd, md, vd, torch.from_numpy(g).cuda(), t, lr, b1, b2, eps)
        g64 = g.astype(np.float64)
        M = b1 * M + (1 - b1) * g64
        V = b2 * V + (1 - b2) * g64 * g64
        P = P - lr * (M / (1 - b1 ** t)) / (np.sqrt(V / (1 - b2 ** t)) + eps)
    torch.cuda.synchronize()
    gmax = max(float(np.abs(g).max()) for g in grads)  # f32 rounding of the terms, which may cancel
    np.testing.assert_allclose(md.cpu().numpy(), M, rtol=1e-5, atol=1e-6 * gmax)
    np.testing.assert_allclose(vd.cpu().numpy(), V, rtol=1e-5, atol=1e-6 * gmax * gmax)
    np.testing.assert_allclose(pd.cpu().numpy(), P, rtol=1e-6, atol=1e-5 * lr * len(grads))  # each update to f32 rounding of m^ / sqrt(v^)


def test_trainer_lowers_the_loss(tmp_path, params):
    import rusty_sr_amd as r
    crops = []
    for name in ("cartoon_rsa.png", "butterfly_rs.png", "logo_nn.png"):
        img = load_png(name)[..., :3]
        crops.append(np.ascontiguousarray(img[:48, :48]))
    crops.append(np.ascontiguousarray(load_png("butterfly_rs.png")[..., :3][-48:, -48:]))
    batch = np.stack(crops)
    start = synthetic_params(2, 5)
    eng = r.Engine(start, device=0, factor=2)
    try:
        tr = r.Trainer(eng, start, l2=1e-6)
        losses = [tr.step(batch) for _ in range(30)]
        final, n_el, _ = eng.backprop(batch, tr.params(), loss_scale=1.0)
        print(f"trainer: err_sum {losses[0]:.6g} -> {final:.6g} after 30 steps ({n_el} elements)")
        assert final < losses[0]
        path = tmp_path / "t.rsr"
        tr.save(str(path))
        assert np.array_equal(r.rsr.decode(path.read_bytes()), tr.params())
    finally:
        eng.close()
