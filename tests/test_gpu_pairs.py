"""LR / HR pairs on the GPU (include/srhip.h "Pairs": sr_pair_validation_error_*, sr_pair_backprop_*, sr_train_add_pair,
sr_train_step_pairs) and `rusty_sr train / validate --lr_folder` end to end.  The paired path is the pooled path with the pool taken
out, so a pair whose LR image is the GPU's own pooled input must give the pooled calls' bits; a u8 LR image is held to img_to_data bit
for bit, to the CPU oracle and to the f64 autograd restatement (tests/grad_ref.py) with the bounds of tests/test_gpu_backprop.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import grad_ref
import oracle
from conftest import ROOT, synth_u8
from test_grad_restatement import synthetic_params

pytestmark = pytest.mark.gpu


def weights(params, f):
    return params["imagenet"] if f == 3 else synthetic_params(f, 100 + f)


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


def with_alpha(px, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.concatenate([px, rng.integers(0, 256, px.shape[:-1] + (1,), dtype=np.uint8)], axis=-1))


def u8_pairs(f, n, lh, lw, seed, lr_ch=3, hr_ch=3):
    """HR: the suite's smoothed noise.  LR: the u8-quantised f64 pool of the HR plus a seeded perturbation of up to 3 levels -- no pool
    reproduces it, and the activations stay in the range the pooled cases cover."""
    hr = synth_u8(seed, n, f * lh, f * lw)
    pooled = grad_ref.pool(grad_ref.hr_values(hr), f).numpy()
    rng = np.random.default_rng(seed + 1)
    lr = np.clip(np.floor(255.0 * pooled + 0.5) + rng.integers(-3, 4, pooled.shape), 0, 255).astype(np.uint8)
    if lr_ch == 4:
        lr = with_alpha(lr, seed + 2)
    if hr_ch == 4:
        hr = with_alpha(hr, seed + 3)
    return np.ascontiguousarray(lr), np.ascontiguousarray(hr)


def lr_as_f32(lr):
    return lr[..., :3].astype(np.float32) / np.float32(255)


def assert_grad_close(g, want, f, what=""):
    """the bounds of tests/test_gpu_backprop.py assert_grad_close, restated"""
    g, want = g.astype(np.float64), want.astype(np.float64)
    for name, (off, n, _) in grad_ref.segments(f).items():
        d, w = g[off:off + n] - want[off:off + n], want[off:off + n]
        floor = 1e-7 * np.abs(want).max()
        print(f"{what} {name}: |d| {np.linalg.norm(d):.3e} of |w| {np.linalg.norm(w):.3e}; max|d| {np.abs(d).max():.3e} of {np.abs(w).max():.3e}")
        assert np.linalg.norm(d) <= 1e-4 * np.linalg.norm(w) + floor, (what, name, np.linalg.norm(d), np.linalg.norm(w))
        assert np.abs(d).max() <= 1e-3 * np.abs(w).max() + floor, (what, name, np.abs(d).max(), np.abs(w).max())


# ---- 1. the paired path is the pooled path with the pool taken out

POOLED_CASES = [  # (factor, n, h, w, linear_loss): f32 HR batches, sizes multiples of f
    (2, 1, 2, 2, False),      # LR 1 x 1
    (2, 4, 16, 18, True),
    (3, 1, 3, 3, True),       # LR 1 x 1
    (3, 4, 21, 24, False),
    (3, 2, 30, 33, True),
    (4, 1, 4, 4, False),      # LR 1 x 1
    (4, 4, 24, 28, True),
    (4, 2, 32, 20, False),
]


@pytest.mark.parametrize("f,n,h,w,linear", POOLED_CASES)
def test_pair_of_the_pooled_input_gives_the_pooled_bits(engines, params, f, n, h, w, linear):
    p = weights(params, f)
    hr = np.random.default_rng(31 * h + w + f).random((n, h, w, 3), dtype=np.float32)
    for precision in ("f32", "split_f16"):
        eng = engines(f, precision)
        lrs = []
        for img in hr:
            want = eng.validation_error(img, linear)
            lr = eng.validation_nodes(h, w)[0]
            got = eng.validation_error_pair(lr, img, linear)
            assert got == want, (precision, got, want)
            assert np.array_equal(eng.validation_nodes(h, w)[0].view(np.uint32), lr.view(np.uint32))  # lr_out: the LR image as given
            lrs.append(lr)
    eng = engines(f)
    lr = np.stack(lrs)
    want = eng.backprop(hr, p, linear_loss=linear, l2=1e-6)
    got = eng.backprop_pair(lr, hr, p, linear_loss=linear, l2=1e-6)
    assert got[0] == want[0] and got[1] == want[1] == n * 3 * h * w
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


# ---- 2. the u8 input stage

@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("lr_ch", [3, 4])
def test_u8_input_is_img_to_data(engines, params, f, lr_ch):
    eng, p = engines(f), weights(params, f)
    rng = np.random.default_rng(17 * f + lr_ch)
    for lh, lw in ((16, 16), (13, 21), (1, 1), (1, 3), (7, 2)):   # value counts 3 lh lw with every remainder mod 4
        lr = rng.integers(0, 256, (lh, lw, lr_ch), dtype=np.uint8)
        if lh * lw >= 256:
            lr.reshape(-1, lr_ch)[:256, 1] = rng.permutation(256).astype(np.uint8)  # all 256 byte values
        hr = synth_u8(5 + lh, 1, f * lh, f * lw)[0]
        want_lr = lr_as_f32(lr)
        for off in range(4):   # the _dev form at buffer offsets 0..3
            buf = torch.zeros(lr.size + 8, dtype=torch.uint8, device="cuda")
            view = buf[off:off + lr.size].view(lh, lw, lr_ch)
            view.copy_(torch.from_numpy(lr))
            hbuf = torch.zeros(hr.size + 8, dtype=torch.uint8, device="cuda")
            hview = hbuf[(off + 1) % 4:(off + 1) % 4 + hr.size].view(f * lh, f * lw, 3)
            hview.copy_(torch.from_numpy(hr))
            err_d = eng.validation_error_pair_dev(view, hview, False)
            torch.cuda.synchronize()
            got_lr, out = eng.validation_nodes(f * lh, f * lw)
            assert np.array_equal(got_lr.view(np.uint32), want_lr.view(np.uint32)), (lh, lw, off)
            d = (out - hr.astype(np.float32) / np.float32(255)).astype(np.float64).ravel()
            assert err_d.item() == pytest.approx(math.fsum(d * d), rel=1e-12)
        err, ne = eng.validation_error_pair(lr, hr, False)
        assert ne == 3 * f * lh * f * lw and err == err_d.item()
        got_lr, out = eng.validation_nodes(f * lh, f * lw)
        assert np.array_equal(got_lr.view(np.uint32), want_lr.view(np.uint32))
        ref = oracle.forward_factor(p, want_lr[None], f)[0]
        print(f"f {f} lr {lh}x{lw}x{lr_ch}: max |gpu - oracle| {np.abs(out - ref).max():.3e}")
        assert np.abs(out - ref).max() <= 1e-4


def test_all_bytes_convert_like_numpy(engines):
    eng = engines(3)
    b = np.arange(256, dtype=np.uint8)
    lr = np.stack([b, b[::-1], np.roll(b, 7)], axis=-1).reshape(16, 16, 3)
    hr = synth_u8(2, 1, 48, 48)[0]
    eng.validation_error_pair(lr, hr)
    got = eng.validation_nodes(48, 48)[0]
    want = lr.astype(np.float32) / np.float32(255)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- 3. u8 pairs against the f64 restatement

U8_CASES = [  # (factor, n, lh, lw, lr_ch, hr_ch, linear)
    (2, 4, 8, 9, 3, 4, True),
    (2, 1, 1, 1, 4, 3, False),
    (3, 2, 10, 11, 4, 4, False),
    (3, 3, 7, 5, 3, 3, True),
    (4, 4, 8, 7, 4, 3, False),
    (4, 1, 6, 6, 3, 4, True),
    (3, 4, 64, 64, 3, 3, False),   # the reference step: 4 crops of 192 x 192
]


@pytest.mark.parametrize("f,n,lh,lw,lr_ch,hr_ch,linear", U8_CASES)
def test_u8_pairs_match_restatement(engines, params, f, n, lh, lw, lr_ch, hr_ch, linear):
    eng, p = engines(f), weights(params, f)
    lr, hr = u8_pairs(f, n, lh, lw, 500 + 13 * lh + lw + f, lr_ch, hr_ch)
    err, ne, g = eng.backprop_pair(lr, hr, p, linear_loss=linear)
    assert ne == n * 3 * f * lh * f * lw and np.isfinite(g).all()
    _, ne_ref, want = grad_ref.backprop(p, hr, f, linear, None, 0.0, x=lr_as_f32(lr).astype(np.float64))
    assert ne_ref == ne
    assert_grad_close(g, want, f, (f, n, lh, lw, lr_ch, hr_ch, linear))
    val = math.fsum(eng.validation_error_pair(lr[i], hr[i], linear)[0] for i in range(n))
    print(f"err_sum {err!r} vs per-image validation {val!r}")
    assert abs(err - val) <= 1e-6 * val, (err, val)


# ---- 4. determinism

def test_pair_bits_are_reproducible(engines, params):
    import rusty_sr_amd as r
    eng, p = engines(3), params["imagenet"]
    lr, hr = u8_pairs(3, 2, 13, 15, 77, 4, 3)
    a = eng.backprop_pair(lr, hr, p, linear_loss=True, l2=1e-6)
    b = eng.backprop_pair(lr, hr, p, linear_loss=True, l2=1e-6)
    assert a[0] == b[0] and np.array_equal(a[2], b[2])
    va = eng.validation_error_pair(lr[0], hr[0], True)
    assert va == eng.validation_error_pair(lr[0], hr[0], True)
    other = r.Engine(p, device=0, factor=3)
    try:
        c = other.backprop_pair(lr, hr, p, linear_loss=True, l2=1e-6)
        assert va == other.validation_error_pair(lr[0], hr[0], True)
    finally:
        other.close()
    assert a[0] == c[0] and np.array_equal(a[2], c[2])
    d = engines(3, "split_f16").backprop_pair(lr, hr, p, linear_loss=True, l2=1e-6)
    assert a[0] == d[0] and np.array_equal(a[2], d[2])
    lr_d, hr_d, p_d = torch.from_numpy(lr).cuda(), torch.from_numpy(hr).cuda(), torch.from_numpy(p).cuda()
    err_d, g_d = eng.backprop_pair_dev(lr_d, hr_d, p_d, linear_loss=True, l2=1e-6)
    v_d = eng.validation_error_pair_dev(lr_d[0].contiguous(), hr_d[0].contiguous(), True)
    torch.cuda.synchronize()
    assert err_d.item() == a[0] and np.array_equal(g_d.cpu().numpy(), a[2])
    assert v_d.item() == va[0]


# ---- 5. the session

def _pair_images(f, seed):
    """pairs with RGB and RGBA members, some LR images smaller than the crop on one or both axes, one of a single pixel"""
    out = []
    for k, (lh, lw, lc, hc) in enumerate([(14, 15, 3, 3), (4, 17, 4, 3), (11, 3, 3, 4), (9, 10, 4, 4), (1, 1, 3, 3), (20, 11, 4, 3)]):
        lr, hr = u8_pairs(f, 1, lh, lw, seed + 10 * k, lc, hc)
        out.append((lr[0], hr[0]))
    return out


def _crop(img, y0, x0, ch, cw):
    out = np.zeros((ch, cw, 3), np.uint8)
    h, w = img.shape[:2]
    ys, xs = max(y0, 0), max(x0, 0)
    ye, xe = min(y0 + ch, h), min(x0 + cw, w)
    if ys < ye and xs < xe:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = img[ys:ye, xs:xe, :3]
    return out


def _pair_plan(n_img, seed, clh, clw):
    """steps of ("pair" | "plain", items): origins inside, negative and overhanging; plain steps crop the HR members"""
    rng = np.random.default_rng(seed)
    steps = []
    for s, n in enumerate([3, 1, 4, 2, 4, 2]):
        kind = "plain" if s in (2, 4) else "pair"
        steps.append((kind, [(int(rng.integers(0, n_img)), int(rng.integers(-clh, 17)), int(rng.integers(-clw, 17))) for _ in range(n)]))
    return steps


def _pair_reference(eng, start, pairs, plan, clh, clw, linear, l2):
    f = eng.factor
    dev = torch.device("cuda", eng.device)
    p = torch.from_numpy(start.copy()).to(dev)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    err = torch.empty(1, dtype=torch.float64, device=dev)
    errs = []
    for t, (kind, items) in enumerate(plan, 1):
        hr = torch.from_numpy(np.stack([_crop(pairs[i][1], f * y0, f * x0, f * clh, f * clw) for i, y0, x0 in items])).to(dev).contiguous()
        if kind == "pair":
            lr = torch.from_numpy(np.stack([_crop(pairs[i][0], y0, x0, clh, clw) for i, y0, x0 in items])).to(dev).contiguous()
            eng.backprop_pair_dev(lr, hr, p, linear, None, l2, grad=g, err=err)
        else:
            eng.backprop_dev(hr, p, linear, None, l2, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
        torch.cuda.synchronize()
        errs.append(float(err.item()))
    return np.array(errs), p.cpu().numpy()


def _pair_session(eng, start, pairs, plan, clh, clw, linear, l2, store_bytes, resident=lambda i: True):
    import rusty_sr_amd as r
    f = eng.factor
    tr = r.Trainer(eng, start, linear_loss=linear, l2=l2, store_bytes=store_bytes)
    try:
        ids = [tr.add_pair(*pr) if resident(i) else -1 for i, pr in enumerate(pairs)]
        plain = [tr.add_image(pr[1]) if resident(i) else -1 for i, pr in enumerate(pairs)]
        for kind, items in plan:
            if kind == "pair":
                tr.step_pair_crops([(ids[i] if ids[i] >= 0 else pairs[i], y0, x0) for i, y0, x0 in items], clh, clw)
            else:
                tr.step_crops([(plain[i] if plain[i] >= 0 else pairs[i][1], f * y0, f * x0) for i, y0, x0 in items], f * clh, f * clw)
        return np.array(tr.sync()), tr.params(), ids
    finally:
        tr.close()


@pytest.mark.parametrize("f,clh,clw,linear", [(2, 9, 11, False), (3, 8, 7, True), (4, 5, 6, False)])
def test_pair_session_steps_equal_backprop_on_numpy_crops(f, clh, clw, linear):
    import rusty_sr_amd as r
    start = synthetic_params(f, 60 + f)
    pairs = _pair_images(f, 20 * f)
    plan = _pair_plan(len(pairs), f, clh, clw)
    eng = r.Engine(start, device=0, factor=f)
    try:
        want_err, want_p = _pair_reference(eng, start, pairs, plan, clh, clw, linear, 1e-6)
        for store, resident, check in ((1 << 30, lambda i: True, lambda ids: min(ids) >= 0),
                                       (0, lambda i: True, lambda ids: max(ids) == -1),
                                       (1 << 30, lambda i: i % 2 == 0, lambda ids: ids[0] >= 0 and ids[1] == -1)):
            got_err, got_p, ids = _pair_session(eng, start, pairs, plan, clh, clw, linear, 1e-6, store, resident)
            assert check(ids), ids
            assert np.array_equal(got_err.view(np.uint64), want_err.view(np.uint64)), (got_err, want_err)
            assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    finally:
        eng.close()


def test_step_pairs_on_a_whole_batch_and_the_ring():
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 19)
    lr, hr = u8_pairs(3, 1, 10, 10, 8)
    eng = r.Engine(start, device=0, factor=3)
    try:
        a = r.Trainer(eng, start, store_bytes=0)
        errs_a = [a.step_pairs(lr, hr) for _ in range(3)]
        a.close()
        b = r.Trainer(eng, start)
        i = b.add_pair(lr[0], hr[0])
        assert i >= 0
        for _ in range(_lib.SR_TRAIN_RING + 5):
            b.step_pair_crops([(i, 0, 0)], 10, 10)
        errs_b = b.sync()
        assert len(errs_b) == _lib.SR_TRAIN_RING + 5
        assert errs_b[:3] == errs_a and errs_b[0] == eng.backprop_pair(lr, hr, start)[0]
        assert b.sync() == []
        b.close()
        # a stored pair counts both images: a budget of one of them alone is no room
        c = r.Trainer(eng, start, store_bytes=(hr[0].size + 255) // 256 * 256)   # (entries are whole 256-byte units)
        assert c.add_pair(lr[0], hr[0]) == -1 and c.add_image(hr[0]) >= 0
        c.close()
    finally:
        eng.close()


# ---- 6. refusals

def test_pair_refusals_leave_outputs_untouched(engines, params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    eng, p = engines(3), params["imagenet"]
    L = _lib.lib()
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lr, hr = u8_pairs(3, 1, 5, 6, 3)
    g = np.full(p.size, 7.0, dtype=np.float32)
    err, ne = C.c_double(5.0), C.c_size_t(3)
    l8, h8 = lr.ctypes.data_as(u8p), hr.ctypes.data_as(u8p)
    bp = lambda ctx, np_, lc, hc, lh, lw: L.sr_pair_backprop_rgba8(ctx, p.ctypes.data_as(fp), np_, l8, lc, h8, hc, 1, lh, lw, 0, 1.0, 0.0,
                                                                   C.byref(err), C.byref(ne), g.ctypes.data_as(fp))
    va = lambda ctx, lc, hc, lh, lw: L.sr_pair_validation_error_rgba8(ctx, l8, lc, h8, hc, lh, lw, 0, C.byref(err), C.byref(ne))
    assert bp(eng._ctx, p.size - 1, 3, 3, 5, 6) == _lib.SR_E_PARAM_COUNT
    for lc, hc, lh, lw in ((3, 3, 0, 6), (3, 3, 5, 0), (3, 3, -1, 6), (2, 3, 5, 6), (3, 5, 5, 6), (1, 4, 5, 6)):
        assert bp(eng._ctx, p.size, lc, hc, lh, lw) == _lib.SR_E_INVALID
        assert va(eng._ctx, lc, hc, lh, lw) == _lib.SR_E_INVALID
    assert (g == 7.0).all() and err.value == 5.0 and ne.value == 3
    # HR not f x LR: the binding refuses (the ABI passes the size once)
    for bad_hr in (hr[0][:-1], hr[0][:, :-3], np.zeros((15, 19, 3), np.uint8)):
        with pytest.raises(r.SrError) as e:
            eng.validation_error_pair(lr[0], np.ascontiguousarray(bad_hr))
        assert e.value.status == _lib.SR_E_INVALID
        with pytest.raises(r.SrError) as e:
            eng.backprop_pair(lr, np.ascontiguousarray(bad_hr)[None], p)
        assert e.value.status == _lib.SR_E_INVALID
    # device forms: misaligned pointers refused before any launch
    lr_d, hr_d = torch.from_numpy(lr).cuda(), torch.from_numpy(hr).cuda()
    p_d = torch.from_numpy(np.concatenate([[0], p]).astype(np.float32)).cuda()
    g_d = torch.full((p.size + 1,), 7.0, device="cuda")
    e_d = torch.full((2,), 5.0, dtype=torch.float64, device="cuda")
    vp = C.c_void_p
    odd = lambda t, b: vp(t.data_ptr() + b)
    dev = lambda pp, ee, gg: L.sr_pair_backprop_rgba8_dev(eng._ctx, pp, vp(lr_d.data_ptr()), 3, vp(hr_d.data_ptr()), 3, 1, 5, 6, 0, 1.0, 0.0,
                                                          ee, gg, None)
    assert dev(odd(p_d, 2), vp(e_d.data_ptr()), vp(g_d.data_ptr())) == _lib.SR_E_INVALID
    assert dev(vp(p_d.data_ptr()), odd(e_d, 2), vp(g_d.data_ptr())) == _lib.SR_E_INVALID
    assert dev(vp(p_d.data_ptr()), vp(e_d.data_ptr()), odd(g_d, 1)) == _lib.SR_E_INVALID
    assert L.sr_pair_validation_error_rgba8_dev(eng._ctx, vp(lr_d.data_ptr()), 3, vp(hr_d.data_ptr()), 3, 5, 6, 0, odd(e_d, 2),
                                                None) == _lib.SR_E_INVALID
    torch.cuda.synchronize()
    assert (g_d.cpu() == 7.0).all() and (e_d.cpu() == 5.0).all()
    bil = r.Engine((), device=0, graph="bilinear")
    try:
        assert bp(bil._ctx, p.size, 3, 3, 5, 6) == _lib.SR_E_INVALID
        assert va(bil._ctx, 3, 3, 5, 6) == _lib.SR_E_INVALID
    finally:
        bil.close()
    assert (g == 7.0).all() and err.value == 5.0
    e2, _, g2 = eng.backprop_pair(lr, hr, p)   # the context is still usable
    assert np.isfinite(g2).all() and e2 > 0 and eng.validation_error_pair(lr[0], hr[0])[0] > 0


def test_invalid_pair_items_are_refused_and_the_session_keeps_working():
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 11)
    lr, hr = u8_pairs(3, 1, 7, 8, 4)
    lr, hr = lr[0], hr[0]
    eng = r.Engine(start, device=0, factor=3)
    try:
        fresh = r.Trainer(eng, start)
        want = (fresh.step_pair_crops([(fresh.add_pair(lr, hr), 0, 0)], 6, 6), fresh.sync())[1]
        fresh.close()
        tr = r.Trainer(eng, start)
        plain = tr.add_image(hr)
        pair = tr.add_pair(lr, hr)
        assert plain >= 0 and pair >= 0 and plain != pair
        bad = [
            ([(pair + 1, 0, 0)], 6, 6),                    # unknown id
            ([(plain, 0, 0)], 6, 6),                       # a plain image is no pair
            ([], 6, 6),
            ([(pair, 0, 0)] * (_lib.SR_TRAIN_MAX_BATCH + 1), 6, 6),
            ([(pair, 0, 0)], 0, 6),                        # crop below one LR pixel
            ([((np.zeros((4, 4, 2), np.uint8), np.zeros((12, 12, 3), np.uint8)), 0, 0)], 6, 6),  # two channels
            ([((np.zeros((4, 4, 3), np.uint8), np.zeros((12, 12, 5), np.uint8)), 0, 0)], 6, 6),
            ([((np.zeros((4, 4, 3), np.uint8), np.zeros((12, 11, 3), np.uint8)), 0, 0)], 6, 6),  # HR not f x LR
            ([(-5, 0, 0)], 6, 6),
        ]
        for items, ch, cw in bad:
            with pytest.raises(r.SrError) as e:
                tr.step_pair_crops(items, ch, cw)
            assert e.value.status == _lib.SR_E_INVALID
        with pytest.raises(r.SrError) as e:   # a pair id where a plain image is asked for
            tr.step_crops([(pair, 0, 0)], 18, 18)
        assert e.value.status == _lib.SR_E_INVALID
        for a, b in ((np.zeros((4, 4, 2), np.uint8), np.zeros((12, 12, 3), np.uint8)), (lr, hr[:-1])):
            with pytest.raises(r.SrError) as e:
                tr.add_pair(a, np.ascontiguousarray(b))
            assert e.value.status == _lib.SR_E_INVALID
        tr.step_pair_crops([(pair, 0, 0)], 6, 6)
        assert tr.sync() == want
        tr.close()
    finally:
        eng.close()


def test_validation_psnr_scores_pairs(engines):
    import rusty_sr_amd as r
    eng = engines(3)
    lr, hr = u8_pairs(3, 3, 9, 12, 40)
    e = [eng.validation_error_pair(lr[i], hr[i]) for i in range(3)]
    want = -10.0 * math.log10(sum(x[0] for x in e) / sum(x[1] for x in e))
    assert r.validation_psnr([eng], list(hr), lr_images=list(lr)) == want
    assert r.validation_psnr([eng], list(hr)) != want


# ---- 7. the CLI end to end

def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=600)


def _psnr_lines(out):
    return [l for l in out.splitlines() if l.startswith("Validation PSNR:\t")]


@pytest.fixture(scope="module")
def pair_folders(tmp_path_factory):
    """HR PNGs, and LR partners made by perturbing the CLI's own -d output (a .PNG partner: the extension is ignored)"""
    from PIL import Image
    root = tmp_path_factory.mktemp("pairs_cli")
    dirs = {k: root / k for k in ("hr", "lr", "vhr", "vlr", "hr2", "lr2")}
    for d in dirs.values():
        d.mkdir()
    rng = np.random.default_rng(12)

    def make(hr_dir, lr_dir, name, h, w, seed, factor_dir=None):
        Image.fromarray(synth_u8(seed, 1, h, w)[0]).save(hr_dir / f"{name}.png")
        tmp = str(root / "down.png")
        res = _run("-d", str(hr_dir / f"{name}.png"), tmp)
        assert res.returncode == 0, res.stderr
        px = np.asarray(Image.open(tmp).convert("RGB")).astype(np.int32)
        px = np.clip(px + rng.integers(-3, 4, px.shape), 0, 255).astype(np.uint8)
        Image.fromarray(px).save(lr_dir / (f"{name}.PNG" if seed % 2 else f"{name}.png"))
        return px

    for k, (h, w) in enumerate([(255, 300), (210, 261), (150, 300), (300, 222)]):   # multiples of 3; one LR below 64 rows
        make(dirs["hr"], dirs["lr"], f"t{k}", h, w, 70 + k)
    for k in range(2):
        make(dirs["vhr"], dirs["vlr"], f"v{k}", 96, 120, 90 + k)
    # factor-2 pairs: the -d output (factor 3) does not fit, so the LR members are a plain 2 x 2 byte mean
    for k in range(2):
        hr = synth_u8(95 + k, 1, 140, 160)[0]
        Image.fromarray(hr).save(dirs["hr2"] / f"s{k}.png")
        lr = hr.reshape(70, 2, 80, 2, 3).astype(np.int32).sum(axis=(1, 3)) // 4
        Image.fromarray(lr.astype(np.uint8)).save(dirs["lr2"] / f"s{k}.png")
    return root, {k: str(v) for k, v in dirs.items()}


def test_cli_train_and_validate_on_pairs(pair_folders):
    import rusty_sr_amd as r
    root, d = pair_folders
    start = os.path.join(ROOT, "rusty_sr_amd", "res", "imagenet.rsr")
    out, again = str(root / "out.rsr"), str(root / "again.rsr")
    args = ["train", "-s", start, "--lr_folder", d["lr"], "-v", d["vhr"], "--val_lr_folder", d["vlr"], "--steps", "5", "--seed", "9"]
    res = _run(*args, out, d["hr"])
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "Beginning Training" and lines[-1] == "Done", lines
    psnr = _psnr_lines(res.stdout)
    assert len(psnr) >= 1
    blob = open(out, "rb").read()
    p = r.rsr.decode(blob)
    assert p.size == 130459 and np.isfinite(p).all() and not np.array_equal(p, r.rsr.decode(open(start, "rb").read()))
    res2 = _run(*args, again, d["hr"])
    assert res2.returncode == 0 and _psnr_lines(res2.stdout) == psnr
    assert open(again, "rb").read() == blob
    # a pooled training from the same start and seed takes other steps
    res3 = _run("train", "-s", start, "--steps", "5", "--seed", "9", str(root / "pooled.rsr"), d["hr"])
    assert res3.returncode == 0 and open(root / "pooled.rsr", "rb").read() != blob
    # every pair transient: the same file
    res4 = _run(*args, "--store", "0", str(root / "transient.rsr"), d["hr"])
    assert res4.returncode == 0, res4.stderr
    assert open(root / "transient.rsr", "rb").read() == blob


def test_cli_pair_checkpoint_scores_like_validate(pair_folders):
    import rusty_sr_amd as r
    from PIL import Image
    root, d = pair_folders
    start = os.path.join(ROOT, "rusty_sr_amd", "res", "imagenet.rsr")
    out = str(root / "one.rsr")
    res = _run("train", "-s", start, "--lr_folder", d["lr"], "-v", d["vhr"], "--val_lr_folder", d["vlr"], "--steps", "1", "--seed", "4",
               out, d["hr"])
    assert res.returncode == 0, res.stderr
    last = _psnr_lines(res.stdout)[-1]
    val = _run("validate", "-c", out, "--lr_folder", d["vlr"], d["vhr"])
    assert val.returncode == 0, val.stderr
    assert _psnr_lines(val.stdout) == [last]
    pooled = _run("validate", "-c", out, d["vhr"])
    assert pooled.returncode == 0 and _psnr_lines(pooled.stdout) != [last]
    # ... and it is the library's paired score of those files
    eng = r.Engine(r.rsr.decode(open(out, "rb").read()), device=0)
    try:
        names = sorted(os.listdir(d["vhr"]))
        hrs = [np.asarray(Image.open(os.path.join(d["vhr"], n)).convert("RGB")) for n in names]
        lrs = [np.asarray(Image.open(os.path.join(d["vlr"], [m for m in os.listdir(d["vlr"]) if m.split(".")[0] == n.split(".")[0]][0]))
                          .convert("RGB")) for n in names]
        want = r.validation_psnr([eng], hrs, lr_images=lrs)
    finally:
        eng.close()
    assert float(last.split("\t")[1]) == pytest.approx(want, rel=1e-6)


def test_cli_train_factor_flag(pair_folders):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    root, d = pair_folders
    n2 = _lib.lib().sr_num_params_factor(2)
    out = str(root / "f2.rsr")
    res = _run("train", "-f", "2", "--steps", "2", "--seed", "1", out, d["hr2"])
    assert res.returncode == 0, res.stderr
    assert r.rsr.decode(open(out, "rb").read()).size == n2
    out_p = str(root / "f2_pairs.rsr")
    res = _run("train", "--factor", "2", "--lr_folder", d["lr2"], "--steps", "2", "--seed", "1", out_p, d["hr2"])
    assert res.returncode == 0, res.stderr
    p = r.rsr.decode(open(out_p, "rb").read())
    assert p.size == n2 and np.isfinite(p).all() and open(out_p, "rb").read() != open(out, "rb").read()


def test_cli_pair_errors(pair_folders):
    from PIL import Image
    root, d = pair_folders
    # factor 3 against factor-2 pairs: the message names the file, both sizes and the factor
    res = _run("train", "--lr_folder", d["lr2"], "--steps", "1", str(root / "x.rsr"), d["hr2"])
    assert res.returncode != 0
    assert "s0.png" in res.stderr and "160x140" in res.stderr and "80x70" in res.stderr and "3 x" in res.stderr, res.stderr
    res = _run("validate", "--lr_folder", d["lr2"], d["hr2"])
    assert res.returncode != 0 and "s0.png" in res.stderr and "160x140" in res.stderr and "80x70" in res.stderr, res.stderr
    # an HR file without a partner is named; an LR file without one is ignored
    lonely = root / "lonely_hr"
    lonely.mkdir()
    for n in os.listdir(d["vhr"]):
        Image.open(os.path.join(d["vhr"], n)).save(lonely / n)
    Image.fromarray(synth_u8(1, 1, 96, 120)[0]).save(lonely / "orphan.png")
    res = _run("validate", "--lr_folder", d["vlr"], str(lonely))
    assert res.returncode != 0 and "orphan.png" in res.stderr and "no LR partner" in res.stderr, res.stderr
    res = _run("train", "--lr_folder", d["vlr"], "--steps", "1", str(root / "x.rsr"), str(lonely))
    assert res.returncode != 0 and "orphan.png" in res.stderr and "no LR partner" in res.stderr, res.stderr
    res = _run("validate", "--lr_folder", d["lr"], d["vhr"])   # the v* files have no partner among the t* files
    assert res.returncode != 0 and "no LR partner" in res.stderr
    extra = _run("validate", "--lr_folder", str(lonely), d["vhr"])   # wrong sizes (LR = HR size), but every HR file has a partner
    assert extra.returncode != 0 and "no LR partner" not in extra.stderr
