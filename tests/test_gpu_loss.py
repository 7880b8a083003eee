"""The training objectives on the GPU (include/srhip.h sr_set_loss: squared, L1, Charbonnier) against their torch-f64 restatement
(tests/loss_ref.py) on inputs whose residuals keep a margin from zero (tests/test_loss_cpu.py asserts the margins on the same tables),
and everything around it: the default's bits, linearity, reproducibility, the training session's steps, the calls that must not look at
the objective, descent, refusals and `rusty_sr train --loss`."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import grad_ref
import loss_ref
from conftest import synth_u8
from test_gpu_augment import _bits_equal, _window
from test_gpu_backprop import assert_grad_close, gpu_pool, validation_err

pytestmark = pytest.mark.gpu

NEW = [("l1", 1e-3), ("charbonnier", 1e-3)]


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision="f32"):
        k = (factor, precision)
        if k not in made:
            made[k] = r.Engine(loss_ref.weights(params, factor), device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def _bits(t):
    return (t[0], t[2].view(np.uint32).tobytes())


def _with_alpha(px, seed):
    a = np.random.default_rng(seed).integers(0, 256, px.shape[:-1] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([px, a], axis=-1))


# ---- against the restatement

@pytest.mark.parametrize("kind,eps", NEW)
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("f,n,lh,lw", loss_ref.PAIR_CASES)
def test_constructed_pairs_match_restatement(engines, params, f, n, lh, lw, linear, kind, eps):
    eng, p = engines(f), loss_ref.weights(params, f)
    eng.set_loss(kind, eps)
    try:
        for target in ("f32", "u8"):
            lr, hr = loss_ref.constructed_pair(p, f, n, lh, lw, loss_ref.pair_seed(lh, lw), target)
            err, ne, g = eng.backprop_pair(lr, hr, p, linear_loss=linear)
            e_ref, ne_ref, want, margin = loss_ref.backprop(p, hr, f, kind, eps, linear, x=loss_ref.lr_values(lr))
            print(f"{kind} f={f} {n}x{lh}x{lw} {target} linear={linear}: min |e| {margin:.3e}, err_sum {err:.9g} (f64 {e_ref:.9g})")
            assert ne == ne_ref and margin >= loss_ref.MARGIN_PAIR and np.isfinite(g).all()
            assert_grad_close(g, want, f, (kind, f, n, lh, lw, target, linear))
            val = sum(eng.validation_error_pair(a, b, linear)[0] for a, b in zip(lr, hr))
            assert abs(err - val) <= 1e-6 * val, (err, val)
    finally:
        eng.set_loss("mse")


@pytest.mark.parametrize("kind,eps", NEW)
@pytest.mark.parametrize("f,n,h,w,linear,seed", loss_ref.POOL_CASES)
def test_pooled_cases_match_restatement(engines, params, f, n, h, w, linear, seed, kind, eps):
    eng, p = engines(f), loss_ref.weights(params, f)
    base = synth_u8(seed, n, h, w)
    lr, _ = gpu_pool(eng, base)   # the GPU's own pooled input, which test_gpu_validation.py holds to its restatement
    eng.set_loss(kind, eps)
    try:
        for hr in (base, _with_alpha(base, seed)):
            err, ne, g = eng.backprop(hr, p, linear_loss=linear)
            _, ne_ref, want, margin = loss_ref.backprop(p, hr, f, kind, eps, linear, x=lr.astype(np.float64))
            assert ne == ne_ref and margin >= loss_ref.MARGIN_POOL, margin   # (on the GPU's own f32 pool: it moves by ~1e-7)
            assert_grad_close(g, want, f, (kind, f, n, h, w, linear, hr.shape[-1]))
            val = validation_err(eng, hr, linear)
            assert abs(err - val) <= 1e-6 * val, (err, val)
    finally:
        eng.set_loss("mse")


@pytest.mark.parametrize("eps", [1e-3, 1e-2])
def test_charbonnier_on_natural_targets(engines, params, eps):
    """smooth in e: no margin needed, so the pooled forms on any seed and an f32 batch"""
    eng, p = engines(3), params["imagenet"]
    eng.set_loss("charbonnier", eps)
    try:
        for hr, linear in ((synth_u8(5, 2, 24, 27), False), (_with_alpha(synth_u8(6, 1, 20, 23), 6), True),
                           (np.random.default_rng(7).random((1, 17, 16, 3), dtype=np.float32), False)):
            err, ne, g = eng.backprop(hr, p, linear_loss=linear)
            lr, _ = gpu_pool(eng, hr)
            _, _, want, _ = loss_ref.backprop(p, hr, 3, "charbonnier", eps, linear, x=lr.astype(np.float64))
            assert_grad_close(g, want, 3, (eps, hr.shape, linear))
            val = validation_err(eng, hr, linear)
            assert abs(err - val) <= 1e-6 * val
    finally:
        eng.set_loss("mse")


# ---- the default

def test_default_is_the_squared_loss_and_reset_gives_its_bits(params):
    import rusty_sr_amd as r
    p = params["imagenet"]
    hr = _with_alpha(synth_u8(11, 2, 40, 44), 11)
    lr, hrp = loss_ref.constructed_pair(p, 3, 2, 8, 9, 3, "u8")
    img = synth_u8(3, 1, 30, 30)[0]

    def run(eng):
        a = eng.backprop(hr, p, linear_loss=True, l2=1e-6)
        b = eng.backprop_pair(lr, hrp, p)
        tr = r.Trainer(eng, p, l2=1e-6, loss=eng.loss[0])
        e = tr.step(img[None])
        q = tr.params()
        tr.close()
        return _bits(a), _bits(b), e, q.view(np.uint32).tobytes()

    fresh, reset = r.Engine(p, device=0), r.Engine(p, device=0)
    try:
        assert fresh.loss == ("mse", pytest.approx(1e-3, rel=1e-6))
        want = run(fresh)
        reset.set_loss("mse")
        assert run(reset) == want
        reset.set_loss("l1")
        assert reset.loss[0] == "l1" and run(reset) != want
        reset.set_loss("charbonnier", 0.25)
        assert reset.loss == ("charbonnier", 0.25)
        reset.set_loss("mse")
        assert reset.loss == ("mse", 0.25) and run(reset) == want
        # the parent's semantics: the restatement of the squared loss
        err, _, g = fresh.backprop(hr, p, linear_loss=True, l2=1e-6)
        pooled, _ = gpu_pool(fresh, hr)
        _, _, ref = grad_ref.backprop(p, hr, 3, True, None, 1e-6, x=pooled.astype(np.float64))
        assert_grad_close(g, ref, 3)
    finally:
        fresh.close()
        reset.close()


@pytest.mark.parametrize("kind,eps", NEW)
def test_scale_and_l2_are_linear(engines, params, kind, eps):
    eng, p = engines(3), params["imagenet"]
    hr = synth_u8(5, 2, 24, 27)
    eng.set_loss(kind, eps)
    try:
        _, _, g1 = eng.backprop(hr, p, loss_scale=1.0, l2=0.0)
        s, lam = 0.37, 0.021
        _, _, g = eng.backprop(hr, p, loss_scale=s, l2=lam)
    finally:
        eng.set_loss("mse")
    want = s * g1.astype(np.float64) + 2 * lam * p.astype(np.float64)
    assert np.linalg.norm(g - want) <= 1e-6 * np.linalg.norm(want)


@pytest.mark.parametrize("kind,eps", NEW)
def test_bits_are_reproducible(engines, params, kind, eps):
    import rusty_sr_amd as r
    eng, p = engines(3), params["imagenet"]
    hr = _with_alpha(synth_u8(11, 2, 40, 44), 11)
    other, split = r.Engine(p, device=0, factor=3), engines(3, "split_f16")
    try:
        for e in (eng, other, split):
            e.set_loss(kind, eps)
        a = eng.backprop(hr, p, linear_loss=True, l2=1e-6)
        assert _bits(eng.backprop(hr, p, linear_loss=True, l2=1e-6)) == _bits(a)
        assert _bits(other.backprop(hr, p, linear_loss=True, l2=1e-6)) == _bits(a)
        assert _bits(split.backprop(hr, p, linear_loss=True, l2=1e-6)) == _bits(a)
        err_d, g_d = eng.backprop_dev(torch.from_numpy(hr).cuda(), torch.from_numpy(p).cuda(), linear_loss=True, l2=1e-6)
        torch.cuda.synchronize()
        assert err_d.item() == a[0] and np.array_equal(g_d.cpu().numpy().view(np.uint32), a[2].view(np.uint32))
    finally:
        other.close()
        eng.set_loss("mse")
        split.set_loss("mse")


# ---- training sessions

F, CROP, BATCH = 3, 12, 2


def _session_images():
    return [synth_u8(21, 1, 30, 34)[0], _with_alpha(synth_u8(22, 1, 26, 29)[0], 22)]


def _chain(eng, start, batches, losses, l2=1e-6):
    """backprop[_pair]_dev + adam_step_dev on numpy batches, batch t under losses[t]: (err_sums, parameters, moments)"""
    dev = torch.device("cuda", eng.device)
    p = torch.from_numpy(start.copy()).to(dev)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    err = torch.empty(1, dtype=torch.float64, device=dev)
    errs = []
    for t, (batch, loss) in enumerate(zip(batches, losses), 1):
        eng.set_loss(*loss)
        if isinstance(batch, tuple):
            eng.backprop_pair_dev(torch.from_numpy(batch[0]).to(dev).contiguous(), torch.from_numpy(batch[1]).to(dev).contiguous(), p, False,
                                  None, l2, grad=g, err=err)
        else:
            eng.backprop_dev(torch.from_numpy(batch).to(dev).contiguous(), p, False, None, l2, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
        torch.cuda.synchronize()
        errs.append(float(err.item()))
    return np.array(errs), p.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("form", ["crops", "members", "pairs", "degraded"])
def test_session_steps_under_l1_equal_the_chained_calls(form):
    """a step of each kind at batch 2, 12 x 12 crops, f = 3 under L1 = backprop[_pair]_dev then adam_step_dev under L1: err_sum and
    parameters bit for bit.  The session keeps its moments to itself, so the step is taken twice: the second update reads the moments
    the first one left, and its parameters match bit for bit only if those did."""
    import rusty_sr_amd as r
    from param_families import bundled_scale
    start = bundled_scale(F, 61)
    imgs = _session_images()
    items = [(0, 5, 7, 0), (1, 3, 2, 0)]
    if form in ("members", "degraded"):
        items = [(0, 5, 7, 3), (1, 3, 2, 6)]
    eng = r.Engine(start, device=0, factor=F)
    try:
        rgb = [im[..., :3] for im in imgs]
        if form == "pairs":
            lrs = [np.ascontiguousarray(synth_u8(31 + i, 1, 10, 11)[0]) for i in range(2)]
            hrs = [np.ascontiguousarray(synth_u8(41 + i, 1, 30, 33)[0]) for i in range(2)]
            pit = [(0, 2, 3), (1, 4, 1)]
            c = CROP // F
            batch = (np.stack([lrs[i][y:y + c, x:x + c] for i, y, x in pit]),
                     np.stack([hrs[i][F * y:F * y + CROP, F * x:F * x + CROP] for i, y, x in pit]))
        elif form == "degraded":
            degs = [dict(sigma=1.2, noise=6.0, quality=70, seed=5), dict(sigma=0.0, noise=0.0, quality=40, seed=9)]
            batch = (np.stack([eng.degrade(imgs[i], F, window=(y, x, CROP, CROP), member=k, **d) for (i, y, x, k), d in zip(items, degs)]),
                     np.stack([_window(rgb[i], y, x, CROP, CROP, k) for i, y, x, k in items]))
        else:
            batch = np.stack([_window(rgb[i], y, x, CROP, CROP, k) for i, y, x, k in items])
        # two steps on the same batch: the second one's update reads the moments the first one left
        want = _chain(eng, start, [batch, batch], [("l1",), ("l1",)])
        tr = r.Trainer(eng, start, l2=1e-6, loss="l1")
        assert eng.loss[0] == "l1"
        ids = [tr.add_pair(lrs[i], hrs[i]) for i in range(2)] if form == "pairs" else [tr.add_image(im) for im in imgs]
        assert min(ids) >= 0
        for _ in range(2):
            if form == "pairs":
                tr.step_pair_crops([(ids[i], y, x) for i, y, x in pit], CROP // F, CROP // F)
            else:
                its = [(ids[i], y, x, k) if form != "crops" else (ids[i], y, x) for i, y, x, k in items]
                if form == "degraded":
                    tr.step_degraded(its, degs, CROP, CROP)
                else:
                    tr.step_crops(its, CROP, CROP)
        got = (np.array(tr.sync()), tr.params())
        tr.close()
        assert _bits_equal(got, want[:2]), (form, got[0], want[0])
        # ... and not what the squared loss gives
        mse = _chain(eng, start, [batch], [("mse",)])
        assert not np.array_equal(mse[1], _chain(eng, start, [batch], [("l1",)])[1])
    finally:
        eng.close()


def test_objective_changed_between_queued_steps():
    """a step under MSE, set_loss("l1") without a sync, a second step: step 1 keeps MSE (its arguments were captured), step 2 is L1"""
    import rusty_sr_amd as r
    from param_families import bundled_scale
    start = bundled_scale(F, 62)
    imgs = _session_images()
    rgb = [im[..., :3] for im in imgs]
    plan = [[(0, 1, 2), (1, 6, 4)], [(1, 0, 9), (0, 11, 3)]]
    batches = [np.stack([np.ascontiguousarray(rgb[i][y:y + CROP, x:x + CROP]) for i, y, x in items]) for items in plan]
    eng = r.Engine(start, device=0, factor=F)
    try:
        want = _chain(eng, start, batches, [("mse",), ("l1",)])
        same = _chain(eng, start, batches, [("mse",), ("mse",)])
        assert not np.array_equal(want[1], same[1])
        tr = r.Trainer(eng, start, l2=1e-6)
        ids = [tr.add_image(im) for im in imgs]
        tr.step_crops([(ids[i], y, x) for i, y, x in plan[0]], CROP, CROP)
        eng.set_loss("l1")   # no sync in between
        tr.step_crops([(ids[i], y, x) for i, y, x in plan[1]], CROP, CROP)
        got = (np.array(tr.sync()), tr.params())
        tr.close()
        assert _bits_equal(got, want[:2]), (got[0], want[0])
    finally:
        eng.close()


# ---- calls that do not look at the objective

def test_validation_metrics_and_inference_ignore_the_objective(params):
    import rusty_sr_amd as r
    p = params["imagenet"]
    hr = synth_u8(8, 1, 48, 51)[0]
    px = synth_u8(9, 1, 20, 23)
    eng = r.Engine(p, device=0)
    try:
        def run():
            return (eng.validation_error(hr, True), eng.validation_error(hr, False), repr(eng.validation_metrics(hr)),
                    eng.upscale_rgba8(px).tobytes())
        before = run()
        eng.set_loss("l1")
        assert run() == before
        eng.set_loss("charbonnier", 1e-2)
        assert run() == before
    finally:
        eng.close()


# ---- descent

@pytest.mark.parametrize("kind,eps", [("l1", 1e-3), ("charbonnier", 1e-3), ("charbonnier", 1e-2)])
def test_trainer_lowers_the_restated_loss(kind, eps):
    """20 steps on one fixed constructed batch lower the f64-restated value of the objective they were taken under"""
    import rusty_sr_amd as r
    from param_families import bundled_scale
    f = 2
    start = bundled_scale(f, 5)
    lr, hr = loss_ref.constructed_pair(start, f, 2, 10, 11, 17, "u8")
    x, target = loss_ref.lr_values(lr), grad_ref.hr_values(hr)

    def value(p):
        with torch.no_grad():
            return float(loss_ref.loss(torch.from_numpy(p.astype(np.float64)), x, target, f, kind, eps, False, 1.0 / target.numel(), 0.0)[0])

    eng = r.Engine(start, device=0, factor=f)
    try:
        tr = r.Trainer(eng, start, l2=1e-6, loss=kind, loss_eps=eps)
        assert eng.loss == (kind, pytest.approx(eps, rel=1e-6))
        errs = [tr.step_pairs(lr, hr) for _ in range(20)]
        end = tr.params()
        tr.close()
        a, b = value(start), value(end)
        print(f"{kind} eps {eps}: restated loss {a:.6g} -> {b:.6g} in 20 steps; err_sum {errs[0]:.6g} -> {errs[-1]:.6g}")
        assert np.isfinite(end).all() and b < a
    finally:
        eng.close()


# ---- refusals

def test_refusals_leave_the_objective_unchanged(params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    L = _lib.lib()
    p = params["imagenet"]
    hr = synth_u8(4, 1, 12, 15)
    eng = r.Engine(p, device=0)
    try:
        eng.set_loss("charbonnier", 0.125)
        before = _bits(eng.backprop(hr, p))
        bad = [(-1, 0.125), (3, 0.125), (7, 0.5)] + [(_lib.SR_LOSS_CHARBONNIER, e) for e in (0.0, -1.0, float("nan"), float("inf"), 1.5)]
        for kind, e in bad:
            assert L.sr_set_loss(eng._ctx, kind, e) == _lib.SR_E_INVALID, (kind, e)
            assert eng.loss == ("charbonnier", 0.125)
        assert _bits(eng.backprop(hr, p)) == before
        for kind in (_lib.SR_LOSS_MSE, _lib.SR_LOSS_L1):   # eps is not read for these kinds, and the stored one stays
            assert L.sr_set_loss(eng._ctx, kind, float("nan")) == _lib.SR_OK
            assert eng.loss[1] == 0.125
        assert L.sr_get_loss(eng._ctx, None, None) == _lib.SR_OK
        for graph in ("bilinear", "downsample"):
            other = r.Engine((), device=0, graph=graph)
            try:
                k, e = C.c_int(9), C.c_float(9.0)
                assert L.sr_set_loss(other._ctx, _lib.SR_LOSS_L1, 1e-3) == _lib.SR_E_INVALID
                assert L.sr_get_loss(other._ctx, C.byref(k), C.byref(e)) == _lib.SR_E_INVALID and k.value == 9 and e.value == 9.0
            finally:
                other.close()
        eng.set_loss("charbonnier", 0.125)
        assert _bits(eng.backprop(hr, p)) == before
    finally:
        eng.close()


# ---- rusty_sr train --loss

def test_cli_train_loss_is_repeatable_and_differs_from_mse(tmp_path):
    from PIL import Image
    from rusty_sr_amd.build import build_host
    folder = tmp_path / "train"
    folder.mkdir()
    for k, (h, w) in enumerate([(200, 230), (210, 196)]):
        Image.fromarray(synth_u8(70 + k, 1, h, w)[0]).save(folder / f"t{k}.png")

    def train(name, *flags):
        out = tmp_path / name
        res = subprocess.run([build_host(), "train", *flags, "--steps", "2", "--seed", "1", str(out), str(folder)], capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0 and res.stdout.splitlines() == ["Beginning Training", "Done"], res.stderr
        return out.read_bytes()

    a, b = train("a.rsr", "--loss", "l1"), train("b.rsr", "--loss", "l1")
    mse, plain = train("m.rsr", "--loss", "mse"), train("p.rsr")
    ch = train("c.rsr", "--loss", "charbonnier:0.01", "-l", "--augment")
    assert a == b and mse == plain and a != mse and ch not in (a, mse)
