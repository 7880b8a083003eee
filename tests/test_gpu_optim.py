"""The optimiser's additions on the GPU (include/srhip.h "Optimiser"): the gradient norm against its numpy restatement bit for bit, the
clipped update against sr_adam_step_dev GPU against GPU, the session against the same calls chained by hand, state() / load_state(),
and `rusty_sr train` resumed against the same run in one go."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import optim_ref
from conftest import ROOT, synth_u8
from test_grad_restatement import synthetic_params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def eng():
    import rusty_sr_amd as r
    e = r.bilinear_net(3, device=0)   # the norm and the update work in any graph's context
    yield e
    e.close()


def _at_offset(x, off):
    """x on the device at a pointer `off` floats past a 256-byte boundary"""
    buf = torch.empty(x.size + 64 + off, dtype=torch.float32, device=DEV)
    base = (-(buf.data_ptr() // 4)) % 64   # floats to the next 256-byte boundary
    view = buf[base + off:base + off + x.size]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 256 == 4 * off
    return view


# ---- the norm
def _factor_sizes():
    from rusty_sr_amd import _lib
    return tuple(_lib.lib().sr_num_params_factor(f) for f in (2, 3, 4))


@pytest.mark.parametrize("n", optim_ref.NORM_SIZES + (117484, 130459, 148624))
def test_norm_equals_the_restatement(eng, n):
    assert (117484, 130459, 148624) == _factor_sizes()
    for name, g in optim_ref.norm_vectors(n).items():
        S = optim_ref.sumsq(g)
        norm = float(np.sqrt(S))
        clips = (0.0, 1.0) if name == "zero" else (0.0, float(np.float32(0.5 * norm)), float(np.float32(2.0 * norm)))
        for off in range(4):
            d_g = _at_offset(g, off)
            for clip in clips:
                if not np.isfinite(np.float32(clip)):
                    continue
                want = optim_ref.grad_norm(g, clip)
                got = eng.read_grad_norm(eng.grad_norm_dev(d_g, clip))
                again = eng.read_grad_norm(eng.grad_norm_dev(d_g, clip))
                assert _same(np.float64(got["sumsq"]), np.float64(want["sumsq"])), (n, name, off, clip, got, want)
                assert _same(np.float32(got["scale"]), np.float32(want["scale"])), (n, name, off, clip, got, want)
                assert got["skip"] == want["skip"] == 0
                assert _same(np.float64(again["sumsq"]), np.float64(got["sumsq"])) and _same(np.float32(again["scale"]), np.float32(got["scale"]))
                if name == "zero":
                    assert got["sumsq"] == 0.0 and got["scale"] == 1.0
                elif clip and clip < norm:
                    assert got["scale"] < 1.0
    # one element that is not finite, first, last and in between: the flag, whatever the rest holds
    g = optim_ref.norm_vectors(n)["gauss"]
    for pos in sorted({0, n // 2, n - 1}):
        for bad in (np.nan, np.inf, -np.inf):
            h = g.copy()
            h[pos] = bad
            got = eng.read_grad_norm(eng.grad_norm_dev(_at_offset(h, pos % 4), 1.0))
            assert got["skip"] == 1, (n, pos, bad, got)
            if np.isnan(bad):
                assert np.isnan(got["sumsq"]) and got["scale"] == 1.0
            else:
                assert got["sumsq"] == np.inf and got["scale"] == 0.0


def test_norm_and_update_refusals(eng):
    import ctypes as C
    from rusty_sr_amd import _lib
    L, ctx = eng._L, eng._ctx
    g = torch.ones(64, dtype=torch.float32, device=DEV)
    out = torch.full((16,), 7, dtype=torch.uint8, device=DEV)
    vp = lambda t, byte_off=0: C.c_void_p(t.data_ptr() + byte_off)
    bad_norm = [(None, 64, 1.0, vp(out)), (vp(g), 64, 1.0, None), (vp(g), 0, 1.0, vp(out)), (vp(g, 2), 32, 1.0, vp(out)),
                (vp(g), 64, 1.0, vp(out, 4)), (vp(g), 64, -1.0, vp(out)), (vp(g), 64, float("nan"), vp(out)), (vp(g), 64, float("inf"), vp(out))]
    for a in bad_norm:
        assert L.sr_grad_norm_dev(ctx, *a, None) == _lib.SR_E_INVALID, a
    p, m, v, e = (torch.ones(64, dtype=torch.float32, device=DEV) for _ in range(4))
    sk = torch.zeros(1, dtype=torch.int64, device=DEV)
    ok = dict(p=vp(p), m=vp(m), v=vp(v), g=vp(g), n=64, step=1, lr=2e-3, norm=None, e=vp(e), d=0.9, sk=vp(sk))
    bad_step = [dict(p=None), dict(m=None), dict(v=None), dict(g=None), dict(n=0), dict(step=0), dict(lr=-1.0), dict(lr=float("nan")),
                dict(p=vp(p, 2)), dict(e=vp(e, 1)), dict(norm=vp(out, 4)), dict(sk=vp(sk, 4)), dict(d=1.0), dict(d=-0.1), dict(d=0.0),
                dict(e=None), dict(d=float("nan"))]
    for change in bad_step:
        a = dict(ok, **change)
        rc = L.sr_adam_step_clipped_dev(ctx, a["p"], a["m"], a["v"], a["g"], a["n"], a["step"], a["lr"], 0.95, 0.995, 1e-7, a["norm"], a["e"],
                                        a["d"], a["sk"], None)
        assert rc == _lib.SR_E_INVALID, change
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7).all() and int(sk.item()) == 0
    for t in (p, m, v, e):
        assert (t.cpu().numpy() == 1.0).all()


# ---- the update, GPU against GPU
UPDATE_CASES = [(5, (0, 0, 0, 0, 0)), (1027, (0, 0, 0, 0, 0)), (1027, (0, 1, 0, 0, 0)), (4099, (0, 0, 0, 3, 0)), (4099, (0, 0, 0, 0, 2)),
                (130459, (0, 0, 0, 0, 0))]   # wide with a tail of 1 and 3, narrow through each kind of pointer, a session's own size


@pytest.mark.parametrize("n,offs", UPDATE_CASES)
def test_update_equals_adam_step_dev(eng, n, offs):
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n).astype(np.float32)
    grads = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for _ in range(3)]
    decay = 0.9
    for mode in ("scale1", "half"):
        p, m, v = _at_offset(p0, offs[0]), _at_offset(np.zeros(n, np.float32), offs[1]), _at_offset(np.zeros(n, np.float32), offs[2])
        e = _at_offset(p0, offs[4])
        rp, rm, rv = (torch.from_numpy(x.copy()).to(DEV) for x in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32)))
        e_ref = p0.copy()
        skipped = torch.zeros(1, dtype=torch.int64, device=DEV)
        for step, g in enumerate(grads, 1):
            d_g = _at_offset(g, offs[3])
            measured = np.sqrt(eng.read_grad_norm(eng.grad_norm_dev(d_g, 0.0))["sumsq"])
            clip = float(np.float32((2.0 if mode == "scale1" else 0.5) * measured))
            norm = eng.grad_norm_dev(d_g, clip)
            scale = np.float32(eng.read_grad_norm(norm)["scale"])
            assert (scale == 1.0) if mode == "scale1" else (0.4 < scale < 0.6)
            eng.adam_step_clipped_dev(p, m, v, d_g, step, norm=norm, ema=e, ema_decay=decay, skipped=skipped)
            eng.adam_step_dev(rp, rm, rv, torch.from_numpy((scale * g).astype(np.float32)).to(DEV), step)
            torch.cuda.synchronize()
            assert _same(p.cpu().numpy(), rp.cpu().numpy()) and _same(m.cpu().numpy(), rm.cpu().numpy()) and _same(v.cpu().numpy(), rv.cpu().numpy())
            e_ref = optim_ref.ema(e_ref, p.cpu().numpy(), decay)
            assert _same(e.cpu().numpy(), e_ref), (mode, step)
        # without a norm: scale 1; without an average: the same p, m, v
        q, qm, qv = (torch.from_numpy(x.copy()).to(DEV) for x in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32)))
        r2, r2m, r2v = (t.clone() for t in (q, qm, qv))
        d_g = _at_offset(grads[0], offs[3])
        eng.adam_step_clipped_dev(q, qm, qv, d_g, 1)
        eng.adam_step_dev(r2, r2m, r2v, d_g.clone(), 1)
        torch.cuda.synchronize()
        assert _same(q.cpu().numpy(), r2.cpu().numpy()) and _same(qm.cpu().numpy(), r2m.cpu().numpy()) and _same(qv.cpu().numpy(), r2v.cpu().numpy())
        # a skipped step: nothing written but the count
        before = [t.cpu().numpy().copy() for t in (p, m, v, e)]
        bad = grads[0].copy()
        bad[n // 3] = np.nan
        d_bad = _at_offset(bad, offs[3])
        norm = eng.grad_norm_dev(d_bad, 1.0)
        assert eng.read_grad_norm(norm)["skip"] == 1
        eng.adam_step_clipped_dev(p, m, v, d_bad, 4, norm=norm, ema=e, ema_decay=decay, skipped=skipped)
        eng.adam_step_clipped_dev(p, m, v, d_bad, 5, norm=norm, ema=e, ema_decay=decay, skipped=skipped)
        torch.cuda.synchronize()
        assert int(skipped.item()) == 2
        for t, b in zip((p, m, v, e), before):
            assert _same(t.cpu().numpy(), b)


# ---- the session
def _crop(img, y0, x0, ch, cw):
    out = np.zeros((ch, cw, 3), np.uint8)
    h, w = img.shape[:2]
    ys, xs, ye, xe = max(y0, 0), max(x0, 0), min(y0 + ch, h), min(x0 + cw, w)
    if ys < ye and xs < xe:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = img[ys:ye, xs:xe, :3]
    return out


def _setup(f):
    start = synthetic_params(f, 60 + f)
    imgs = [synth_u8(20 * f + k, 1, 12 * f + k, 11 * f + 2 * k)[0] for k in range(3)]
    rng = np.random.default_rng(f)
    c = 8 * f
    plan = [[(int(rng.integers(0, 3)), int(rng.integers(-2, 4 * f)), int(rng.integers(-2, 3 * f))) for _ in range(2)] for _ in range(5)]
    return start, imgs, plan, c


def _schedule():
    import rusty_sr_amd as r
    return r.parse_lr_schedule("cosine:4:1e-4", 2e-3, 2)


def _chain(eng, start, imgs, plan, c, clip, decay, sched):
    """backprop_dev + grad_norm_dev + adam_step_clipped_dev by hand"""
    import rusty_sr_amd as r
    p = torch.from_numpy(start.copy()).to(DEV)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    e = p.clone()
    err = torch.empty(1, dtype=torch.float64, device=DEV)
    stats = []
    for t, items in enumerate(plan, 1):
        hr = torch.from_numpy(np.stack([_crop(imgs[i], y0, x0, c, c) for i, y0, x0 in items])).to(DEV).contiguous()
        eng.backprop_dev(hr, p, False, None, 1e-6, grad=g, err=err)
        norm = eng.grad_norm_dev(g, clip)
        lr = r.lr_at(sched, t)
        eng.adam_step_clipped_dev(p, m, v, g, t, lr=lr, norm=norm, ema=e, ema_decay=decay)
        torch.cuda.synchronize()
        nd = eng.read_grad_norm(norm)
        stats.append({"err_sum": float(err.item()), "grad_norm": float(np.sqrt(nd["sumsq"])), "lr": lr, "scale": nd["scale"]})
    return stats, p.cpu().numpy(), e.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()


def _run_steps(tr, ids, plan, c, sched, first=1):
    import rusty_sr_amd as r
    for t, items in enumerate(plan, first):
        if sched is not None:
            tr.set_lr(r.lr_at(sched, t))
        tr.step_crops([(ids[i], y0, x0) for i, y0, x0 in items], c, c)


@pytest.mark.parametrize("f", [2, 3, 4])
def test_session_with_the_options_off_keeps_the_default_bits(f):
    import rusty_sr_amd as r
    start, imgs, plan, c = _setup(f)
    eng = r.Engine(start, device=0, factor=f)
    try:
        results = []
        for kind in ("default", "set_optim(0, 0)", "set_lr"):
            tr = r.Trainer(eng, start, lr=1e-3 if kind == "set_lr" else 2e-3)
            ids = [tr.add_image(im) for im in imgs]
            if kind == "set_optim(0, 0)":
                tr.set_optim(0.0, 0.0)
            if kind == "set_lr":
                tr.set_lr(2e-3)
            _run_steps(tr, ids, plan, c, None)
            stats = tr.sync_stats() if kind != "default" else None
            errs = [s["err_sum"] for s in stats] if stats is not None else tr.sync()
            if stats is not None:
                assert all(s["grad_norm"] == 0.0 and s["scale"] == 1.0 and np.float32(s["lr"]) == np.float32(2e-3) for s in stats)
            st = tr.state()
            assert st["e"] is None and st["step"] == 5 and st["skipped"] == 0
            results.append((np.array(errs), tr.params(), st["m"], st["v"]))
            tr.close()
        for other in results[1:]:
            for a, b in zip(results[0], other):
                assert _same(a, b)
    finally:
        eng.close()


@pytest.mark.parametrize("f", [2, 3, 4])
def test_session_equals_the_chain_and_resumes(f):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start, imgs, plan, c = _setup(f)
    sched, decay = _schedule(), 0.9
    eng = r.Engine(start, device=0, factor=f)
    try:
        free, *_ = _chain(eng, start, imgs, plan, c, 0.0, decay, sched)
        clip = float(np.float32(0.75 * np.median([s["grad_norm"] for s in free])))
        want, want_p, want_e, want_m, want_v = _chain(eng, start, imgs, plan, c, clip, decay, sched)
        print(f"factor {f}: clip {clip}, scales {[s['scale'] for s in want]}")
        assert any(s["scale"] < 1.0 for s in want)
        # the session, uninterrupted
        a = r.Trainer(eng, start, clip_norm=clip, ema_decay=decay)
        ids = [a.add_image(im) for im in imgs]
        _run_steps(a, ids, plan, c, sched)
        got = a.sync_stats()
        assert len(got) == 5 and a.sync_stats() == []
        for gs, ws in zip(got, want):
            assert _same(np.float64(gs["err_sum"]), np.float64(ws["err_sum"])) and _same(np.float64(gs["grad_norm"]), np.float64(ws["grad_norm"]))
            assert _same(np.float32(gs["scale"]), np.float32(ws["scale"])) and _same(np.float32(gs["lr"]), np.float32(ws["lr"]))
        st_a = a.state()
        assert _same(a.params(), want_p) and _same(a.ema(), want_e) and _same(st_a["m"], want_m) and _same(st_a["v"], want_v)
        assert _same(st_a["e"], want_e) and st_a["step"] == 5 and st_a["skipped"] == 0
        a.close()
        # three steps, state() -> a new session -> load_state() -> the other two
        b = r.Trainer(eng, start, clip_norm=clip, ema_decay=decay)
        ids = [b.add_image(im) for im in imgs]
        _run_steps(b, ids, plan[:3], c, sched)
        st, p3 = b.state(), b.params()
        assert st["step"] == 3
        b.close()
        cont = r.Trainer(eng, p3, clip_norm=clip, ema_decay=decay)
        ids = [cont.add_image(im) for im in imgs]
        # refusals leave the session as it was
        for bad in (dict(st, m=st["m"][:-1], v=st["v"][:-1], e=st["e"][:-1]), dict(st, step=-1), dict(st, skipped=-1), dict(st, e=None)):
            with pytest.raises(r.SrError) as ex:
                cont.load_state(bad)
            assert ex.value.status == _lib.SR_E_INVALID
        for call in (lambda: cont.set_optim(-1.0, decay), lambda: cont.set_optim(clip, 1.0), lambda: cont.set_optim(float("nan"), decay),
                     lambda: cont.set_optim(clip, -0.5), lambda: cont.set_lr(-1.0), lambda: cont.set_lr(float("inf")), lambda: cont.set_lr(float("nan"))):
            with pytest.raises(r.SrError) as ex:
                call()
            assert ex.value.status == _lib.SR_E_INVALID
        assert cont.state()["step"] == 0
        cont.load_state(st)
        _run_steps(cont, ids, plan[3:], c, sched, first=4)
        tail = cont.sync_stats()
        assert len(tail) == 2   # (all four fields: the ring's slots follow the step count that load_state rewrote)
        for gs, ws in zip(tail, want[3:]):
            assert _same(np.float64(gs["err_sum"]), np.float64(ws["err_sum"])) and _same(np.float64(gs["grad_norm"]), np.float64(ws["grad_norm"]))
            assert _same(np.float32(gs["scale"]), np.float32(ws["scale"])) and _same(np.float32(gs["lr"]), np.float32(ws["lr"]))
        st_c = cont.state()
        assert _same(cont.params(), want_p) and _same(cont.ema(), want_e) and _same(st_c["m"], want_m) and _same(st_c["v"], want_v)
        assert st_c["step"] == 5
        # the average off: ema() refuses, and on again it starts at the parameters
        cont.set_optim(clip, 0.0)
        with pytest.raises(r.SrError) as ex:
            cont.ema()
        assert ex.value.status == _lib.SR_E_INVALID
        cont.set_optim(clip, decay)
        assert _same(cont.ema(), cont.params())
        cont.close()
    finally:
        eng.close()


def test_session_skips_a_step_whose_gradient_is_not_finite():
    """A parameter set to NaN makes every gradient NaN: the step is skipped, counted, and nothing moves."""
    import rusty_sr_amd as r
    start, imgs, plan, c = _setup(3)
    poisoned = start.copy()
    poisoned[100] = np.nan
    eng = r.Engine(start, device=0, factor=3)
    try:
        tr = r.Trainer(eng, poisoned, clip_norm=1.0, ema_decay=0.9)
        ids = [tr.add_image(im) for im in imgs]
        _run_steps(tr, ids, plan[:2], c, None)
        stats = tr.sync_stats()
        st = tr.state()
        assert st["skipped"] == 2 and st["step"] == 2 and all(not np.isfinite(s["grad_norm"]) for s in stats)
        assert _same(tr.params(), poisoned) and not st["m"].any() and not st["v"].any() and _same(st["e"], poisoned)
        tr.close()
    finally:
        eng.close()


def test_session_outliving_its_context_refuses_the_new_calls():
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start, imgs, plan, c = _setup(3)
    eng = r.Engine(start, device=0, factor=3)
    tr = r.Trainer(eng, start, clip_norm=1.0, ema_decay=0.9)
    st = tr.state()
    eng.close()
    for call in (lambda: tr.set_optim(1.0, 0.9), lambda: tr.set_lr(1e-3), tr.ema, tr.state, lambda: tr.load_state(st), tr.sync_stats):
        with pytest.raises(r.SrError) as ex:
            call()
        assert ex.value.status == _lib.SR_E_INVALID
    tr.close()


# ---- rusty_sr train: a resumed run against the same run in one go
def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=600)


def _psnr_lines(out):
    return [l for l in out.splitlines() if l.startswith("Validation PSNR")]


RECIPE = ["--seed", "7", "--ema", "0.99", "--lr-schedule", "cosine:200", "--warmup", "10", "--augment"]


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("optim_cli")
    tr, va = root / "train", root / "val"
    tr.mkdir()
    va.mkdir()
    sizes = [(256, 300), (210, 260), (150, 300), (300, 220), (240, 240), (200, 330)]  # one below 192 rows
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(synth_u8(70 + k, 1, h, w)[0]).save(tr / f"t{k}.png")
    for k in range(2):
        Image.fromarray(synth_u8(90 + k, 1, 96, 120)[0]).save(va / f"v{k}.png")
    return root, str(tr), str(va)


@pytest.fixture(scope="module")
def clip_norm(folders):
    """C from a first --timing run that clips nothing (a norm no gradient reaches): the median norm of its 200 steps."""
    root, tr, va = folders
    res = _run("train", str(root / "probe.rsr"), tr, "--steps", "200", "--clip", "1e30", "--timing", *RECIPE)
    assert res.returncode == 0, res.stderr
    m = re.search(r"clipped steps ([\d.]+) %, skipped steps ([\d.]+) %; gradient norm min (\S+), median (\S+), max (\S+)\n", res.stderr)
    assert m, res.stderr
    assert float(m.group(1)) == 0.0 and float(m.group(2)) == 0.0
    lo, med, hi = (float(m.group(k)) for k in (3, 4, 5))
    assert 0.0 < lo <= med <= hi
    return repr(med)


def test_cli_resumed_run_equals_the_run_in_one_go(folders, clip_norm):
    import rusty_sr_amd as r
    root, tr, va = folders
    opts = ["--clip", clip_norm, *RECIPE, "-v", va]
    one, two = str(root / "one.rsr"), str(root / "two.rsr")
    a = _run("train", one, tr, "--steps", "200", "--timing", *opts)
    assert a.returncode == 0, a.stderr
    m = re.search(r"clipped steps ([\d.]+) %, skipped steps ([\d.]+) %", a.stderr)
    print(f"--clip {clip_norm}: {m.group(0)}")
    assert 0.0 < float(m.group(1)) < 100.0   # some steps clip, some do not
    b1 = _run("train", two, tr, "--steps", "100", *opts)
    assert b1.returncode == 0, b1.stderr
    b2 = _run("train", two, tr, "--steps", "200", "--resume", *opts)
    assert b2.returncode == 0, b2.stderr
    for suffix in (".rsr", ".ema.rsr", ".rsr.state"):
        x, y = (open(str(root / (name + suffix)), "rb").read() for name in ("one", "two"))
        assert x == y and len(x) > 0, suffix
    lines = _psnr_lines(a.stdout)
    assert len(lines) == 6 and [l.split(":")[0] for l in lines] == ["Validation PSNR", "Validation PSNR (EMA)"] * 3, lines
    assert lines == _psnr_lines(b1.stdout) + _psnr_lines(b2.stdout) and len(_psnr_lines(b2.stdout)) == 2
    raw, avg = r.rsr.decode(open(one, "rb").read()), r.rsr.decode(open(str(root / "one.ema.rsr"), "rb").read())
    assert raw.size == avg.size == 130459 and np.isfinite(avg).all() and not np.array_equal(raw, avg)
    # a changed option: refused by name, nothing written
    before = open(two, "rb").read()
    for extra, named in ((["--seed", "8"], "--seed"), (["--loss", "l1"], "--loss")):
        args = [o for o in opts if extra[0] != "--seed" or o not in ("--seed", "7")]
        res = _run("train", two, tr, "--steps", "300", "--resume", *args, *extra)
        assert res.returncode == 2 and f"'{named}' differs" in res.stderr, res.stderr
    assert open(two, "rb").read() == before


def test_cli_default_run_is_the_run_with_the_defaults_spelled_out(folders):
    root, tr, va = folders
    a, b = str(root / "default.rsr"), str(root / "spelled.rsr")
    ra = _run("train", a, tr, "-v", va, "--steps", "3", "--seed", "5")
    rb = _run("train", b, tr, "-v", va, "--steps", "3", "--seed", "5", "--lr", "2e-3", "--lr-schedule", "constant")
    assert ra.returncode == 0 and rb.returncode == 0, ra.stderr + rb.stderr
    assert open(a, "rb").read() == open(b, "rb").read() and ra.stdout == rb.stdout
    assert ra.stdout.splitlines() == ["Beginning Training", _psnr_lines(ra.stdout)[0], "Done"]
    assert open(a + ".state", "rb").read() == open(b + ".state", "rb").read()
    assert not os.path.exists(str(root / "default.ema.rsr"))
