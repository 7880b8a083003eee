"""The training session on the GPU (include/srhip.h sr_train_*, sr_set_params) and `rusty_sr train` end to end.  A session step must be
bit-identical to the same crops cut and zero-padded in numpy and run through sr_backprop_rgba8_dev + sr_adam_step_dev."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, synth_u8
from test_grad_restatement import synthetic_params

pytestmark = pytest.mark.gpu


def _images(seed):
    """RGB and RGBA sources, some smaller than the crop on one or both axes, one of a single pixel."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w, c) in enumerate([(40, 45, 3), (12, 50, 4), (31, 9, 3), (26, 29, 4), (1, 1, 3), (60, 33, 4)]):
        px = synth_u8(seed + k, 1, h, w)[0]
        if c == 4:
            px = np.concatenate([px, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
        out.append(np.ascontiguousarray(px))
    return out


def _crop(img, y0, x0, ch, cw):
    """numpy: the crop_h x crop_w x 3 window at (y0, x0), zero outside the image, alpha dropped"""
    out = np.zeros((ch, cw, 3), np.uint8)
    h, w = img.shape[:2]
    ys, xs = max(y0, 0), max(x0, 0)
    ye, xe = min(y0 + ch, h), min(x0 + cw, w)
    if ys < ye and xs < xe:
        out[ys - y0:ye - y0, xs - x0:xe - x0] = img[ys:ye, xs:xe, :3]
    return out


def _plan(n_img, seed, ch, cw):
    """5 steps of 1-4 items with origins inside, negative and overhanging"""
    rng = np.random.default_rng(seed)
    steps = []
    for s in range(5):
        n = [3, 1, 4, 2, 4][s]
        steps.append([(int(rng.integers(0, n_img)), int(rng.integers(-ch, 50)), int(rng.integers(-cw, 50))) for _ in range(n)])
    return steps


def _reference(eng, start, imgs, plan, ch, cw, linear, l2):
    dev = torch.device("cuda", eng.device)
    p = torch.from_numpy(start.copy()).to(dev)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    err = torch.empty(1, dtype=torch.float64, device=dev)
    errs = []
    for t, items in enumerate(plan, 1):
        batch = np.stack([_crop(imgs[i], y0, x0, ch, cw) for i, y0, x0 in items])
        hr = torch.from_numpy(batch).to(dev).contiguous()
        eng.backprop_dev(hr, p, linear, None, l2, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
        torch.cuda.synchronize()
        errs.append(float(err.item()))
    return np.array(errs), p.cpu().numpy()


def _session(eng, start, imgs, plan, ch, cw, linear, l2, store_bytes, resident=lambda i: True):
    import rusty_sr_amd as r
    tr = r.Trainer(eng, start, linear_loss=linear, l2=l2, store_bytes=store_bytes)
    try:
        ids = [tr.add_image(im) if resident(i) else -1 for i, im in enumerate(imgs)]
        for items in plan:
            tr.step_crops([(ids[i] if ids[i] >= 0 else imgs[i], y0, x0) for i, y0, x0 in items], ch, cw)
        errs = tr.sync()
        return np.array(errs), tr.params(), ids
    finally:
        tr.close()


CASES = [(2, 19, 23, False), (3, 24, 19, True), (4, 21, 26, False)]  # crop bytes not a multiple of 4 in two of them


@pytest.mark.parametrize("f,ch,cw,linear", CASES)
def test_session_steps_equal_backprop_on_numpy_crops(f, ch, cw, linear):
    import rusty_sr_amd as r
    start = synthetic_params(f, 40 + f)
    imgs = _images(10 * f)
    plan = _plan(len(imgs), f, ch, cw)
    eng = r.Engine(start, device=0, factor=f)
    try:
        want_err, want_p = _reference(eng, start, imgs, plan, ch, cw, linear, 1e-6)
        got_err, got_p, ids = _session(eng, start, imgs, plan, ch, cw, linear, 1e-6, 1 << 30)
        assert min(ids) >= 0
        assert np.array_equal(got_err.view(np.uint64), want_err.view(np.uint64)), (got_err, want_err)
        assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
        # every image transient, and a mixed store (every other image resident): the same bits
        t_err, t_p, ids = _session(eng, start, imgs, plan, ch, cw, linear, 1e-6, 0)
        assert max(ids) == -1
        assert np.array_equal(t_err.view(np.uint64), want_err.view(np.uint64))
        assert np.array_equal(t_p.view(np.uint32), want_p.view(np.uint32))
        m_err, m_p, ids = _session(eng, start, imgs, plan, ch, cw, linear, 1e-6, 1 << 30, resident=lambda i: i % 2 == 0)
        assert ids[0] >= 0 and ids[1] == -1
        assert np.array_equal(m_err.view(np.uint64), want_err.view(np.uint64))
        assert np.array_equal(m_p.view(np.uint32), want_p.view(np.uint32))
    finally:
        eng.close()


def test_step_on_a_whole_batch_and_the_ring():
    """Trainer.step (a whole batch, synchronous) and more queued steps than the ring holds: every err_sum comes back, in order."""
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 9)
    img = synth_u8(3, 1, 30, 30)[0]
    eng = r.Engine(start, device=0, factor=3)
    try:
        a = r.Trainer(eng, start, store_bytes=0)
        errs_a = [a.step(img[None]) for _ in range(3)]
        a.close()
        b = r.Trainer(eng, start)
        i = b.add_image(img)
        for _ in range(_lib.SR_TRAIN_RING + 5):
            b.step_crops([(i, 0, 0)], 30, 30)
        errs_b = b.sync()
        assert len(errs_b) == _lib.SR_TRAIN_RING + 5
        assert errs_b[:3] == errs_a
        assert b.sync() == []
        b.close()
    finally:
        eng.close()


def test_invalid_items_are_refused_and_the_session_keeps_working():
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 11)
    img = synth_u8(5, 1, 20, 20)[0]
    eng = r.Engine(start, device=0, factor=3)
    try:
        fresh = r.Trainer(eng, start)
        want = (fresh.step_crops([(fresh.add_image(img), 0, 0)], 18, 18), fresh.sync())[1]
        fresh.close()
        tr = r.Trainer(eng, start)
        i = tr.add_image(img)
        bad = [
            ([(i + 1, 0, 0)], 18, 18),                     # unknown id
            ([], 18, 18),                                  # n = 0
            ([(i, 0, 0)] * (_lib.SR_TRAIN_MAX_BATCH + 1), 18, 18),
            ([(i, 0, 0)], 2, 18),                          # crop smaller than the factor
            ([(np.zeros((4, 4, 2), np.uint8), 0, 0)], 18, 18),  # two channels
            ([(-5, 0, 0)], 18, 18),
        ]
        for items, ch, cw in bad:
            with pytest.raises(r.SrError) as e:
                tr.step_crops(items, ch, cw)
            assert e.value.status == _lib.SR_E_INVALID
        with pytest.raises(r.SrError) as e:
            tr.add_image(np.zeros((4, 4, 2), np.uint8))
        assert e.value.status == _lib.SR_E_INVALID
        tr.step_crops([(i, 0, 0)], 18, 18)
        assert tr.sync() == want
        tr.close()
    finally:
        eng.close()


def test_session_outliving_its_context():
    """sr_destroy of the context first: the session is detached (its calls refuse), destroying it later touches nothing of the
    context, and the next context's calls see no error left behind."""
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 13)
    img = synth_u8(6, 1, 24, 24)[0]
    eng = r.Engine(start, device=0, factor=3)
    tr = r.Trainer(eng, start)
    tr.step_crops([(tr.add_image(img), 0, 0)], 24, 24)  # still in flight when the context goes
    eng.close()
    with pytest.raises(r.SrError) as e:
        tr.sync()
    assert e.value.status == _lib.SR_E_INVALID
    tr.close()
    eng2 = r.Engine(start, device=0, factor=3)
    try:
        x = r.img_to_data(img[None])
        assert np.isfinite(eng2.upscale_f32(x)).all()
    finally:
        eng2.close()


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_set_params_equals_a_fresh_context(params, precision):
    import rusty_sr_amd as r
    a, b = params["anime"], params["imagenet"]
    rng = np.random.default_rng(3)
    shapes = [(40, 70), (268, 1024)]
    pxs = [rng.integers(0, 256, (1, h, w, 3), dtype=np.uint8) for h, w in shapes]
    fresh = r.Engine(b, device=0, precision=precision)
    reset = r.Engine(a, device=0, precision=precision)
    try:
        reset.set_params(b)
        for px in pxs:
            x = r.img_to_data(px)
            assert np.array_equal(reset.upscale_f32(x).view(np.uint32), fresh.upscale_f32(x).view(np.uint32))
            assert np.array_equal(reset.upscale_rgba8(px), fresh.upscale_rgba8(px))
    finally:
        fresh.close()
        reset.close()


def test_set_params_checks_like_create(params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    b = params["imagenet"]
    big = b.copy()
    big[5000] = 70000.0
    px = np.random.default_rng(4).integers(0, 256, (1, 40, 70, 3), dtype=np.uint8)
    eng = r.Engine(params["anime"], device=0)
    try:
        eng.set_params(big)
        with pytest.raises(r.SrError) as e:  # as sr_create with that vector: the split-half mode is refused
            eng.set_precision("split_f16")
        assert e.value.status == _lib.SR_E_DOMAIN
        eng.set_params(b)
        eng.set_precision("split_f16")
        with pytest.raises(r.SrError) as e:  # already in that mode: the vector is refused, the weights stay
            eng.set_params(big)
        assert e.value.status == _lib.SR_E_DOMAIN
        before = eng.upscale_rgba8(px)
        with pytest.raises(r.SrError) as e:
            eng.set_params(b[:-1])
        assert e.value.status == _lib.SR_E_PARAM_COUNT
        assert np.array_equal(eng.upscale_rgba8(px), before)
        eng.set_precision("f32")
        ref = r.Engine(b, device=0)
        assert np.array_equal(eng.upscale_rgba8(px), ref.upscale_rgba8(px))
        ref.close()
    finally:
        eng.close()


# ---- rusty_sr train end to end

def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    from PIL import Image
    root = tmp_path_factory.mktemp("train_cli")
    tr, va = root / "train", root / "val"
    tr.mkdir()
    va.mkdir()
    sizes = [(256, 300), (210, 260), (150, 300), (300, 220), (240, 240), (200, 330)]  # one below 192 rows
    for k, (h, w) in enumerate(sizes):
        Image.fromarray(synth_u8(70 + k, 1, h, w)[0]).save(tr / f"t{k}.png")
    for k in range(2):
        Image.fromarray(synth_u8(90 + k, 1, 96, 120)[0]).save(va / f"v{k}.png")
    return root, str(tr), str(va)


def _psnr_lines(out):
    return [l for l in out.splitlines() if l.startswith("Validation PSNR:\t")]


def test_cli_train_end_to_end(folders):
    import rusty_sr_amd as r
    root, tr, va = folders
    out = str(root / "out.rsr")
    res = _run("train", out, tr, "-v", va, "--steps", "101", "--seed", "7")
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "Beginning Training" and lines[-1] == "Done" and len(lines) == 4, lines
    psnr = _psnr_lines(res.stdout)
    assert len(psnr) == 2
    first, second = (float(l.split("\t")[1]) for l in psnr)
    print(f"train CLI: PSNR {first} after step 1, {second} after step 100")
    assert second > first  # from a random start, 100 steps of Adam on the generated set
    blob = open(out, "rb").read()
    p = r.rsr.decode(blob)
    assert p.size == 130459 and np.isfinite(p).all()
    again = str(root / "again.rsr")
    res2 = _run("train", again, tr, "-v", va, "--steps", "101", "--seed", "7")
    assert res2.returncode == 0 and _psnr_lines(res2.stdout) == psnr
    assert open(again, "rb").read() == blob  # the same seed: the same file


def test_cli_train_checkpoint_scores_like_validate(folders):
    root, tr, va = folders
    out = str(root / "out100.rsr")
    res = _run("train", out, tr, "-v", va, "--steps", "100", "--seed", "11")
    assert res.returncode == 0, res.stderr
    last = _psnr_lines(res.stdout)[-1]
    val = _run("validate", "-c", out, va)
    assert val.returncode == 0, val.stderr
    assert _psnr_lines(val.stdout) == [last]


def test_cli_train_from_start_parameters(folders):
    import rusty_sr_amd as r
    root, tr, va = folders
    out = str(root / "from_imagenet.rsr")
    start = os.path.join(ROOT, "rusty_sr_amd", "res", "imagenet.rsr")
    res = _run("train", "-s", start, out, tr, "--steps", "1", "--seed", "3")
    assert res.returncode == 0, res.stderr
    assert res.stdout.splitlines() == ["Beginning Training", "Done"]
    got, ref = r.rsr.decode(open(out, "rb").read()), r.rsr.decode(open(start, "rb").read())
    assert got.size == ref.size and np.isfinite(got).all() and not np.array_equal(got, ref)
    # every image transient (--store 0): the same file as with the store; --timing reports the resident share
    res = _run("train", "-s", start, str(root / "t.rsr"), tr, "--steps", "1", "--seed", "3", "--store", "0", "--timing")
    assert res.returncode == 0 and "steps/s" in res.stderr and re.search(r"resident draws 0\.0 %", res.stderr), res.stderr
    assert open(root / "t.rsr", "rb").read() == open(out, "rb").read()
