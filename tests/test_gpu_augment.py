"""Augmented training steps on the GPU (include/srhip.h sr_train_step_aug / sr_train_step_pairs_aug) and `rusty_sr train --augment`.
An augmented step must be bit-identical to sr_backprop_rgba8_dev (sr_pair_backprop_rgba8_dev) + sr_adam_step_dev on crops that numpy
cut from the item's window and transformed with ensemble_ref.T; the CLI's file must equal a Trainer driven with the CLI's draws,
restated here."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import synth_u8
from ensemble_ref import T
from test_gpu_pairs import _pair_images
from test_gpu_train import _crop, _images
from test_grad_restatement import synthetic_params

pytestmark = pytest.mark.gpu


def _window(img, y0, x0, ch, cw, k):
    """item of the batch: T_k of the window at (y0, x0), which is cw x ch (rows x columns) when k swaps the axes"""
    wh, ww = (cw, ch) if k & 4 else (ch, cw)
    out = T(_crop(img, y0, x0, wh, ww), k)
    assert out.shape == (ch, cw, 3)
    return out


def _plan(n_img, seed, ch, cw, lo=50):
    """5 steps of 1-4 items (image, y0, x0, member): origins inside, negative and overhanging; the 14 members hold all eight, shuffled,
    so that they are mixed within a batch"""
    rng = np.random.default_rng(seed)
    ks = list(rng.permutation(np.concatenate([np.arange(8), rng.integers(0, 8, 6)])))
    assert set(ks) == set(range(8))
    steps = []
    for n in [3, 1, 4, 2, 4]:
        steps.append([(int(rng.integers(0, n_img)), int(rng.integers(-ch, lo)), int(rng.integers(-cw, lo)), int(ks.pop())) for _ in range(n)])
    assert any(len({k for *_, k in items}) > 1 for items in steps)
    return steps


def _bits_equal(got, want):
    return (np.array_equal(np.asarray(got[0]).view(np.uint64), np.asarray(want[0]).view(np.uint64))
            and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)))


def _reference(eng, start, imgs, plan, ch, cw, linear, l2, paired=False):
    """backprop + Adam on numpy crops.  paired: imgs are (lr, hr), ch / cw and the origins in LR pixels"""
    f = eng.factor
    dev = torch.device("cuda", eng.device)
    p = torch.from_numpy(start.copy()).to(dev)
    m, v, g = torch.zeros_like(p), torch.zeros_like(p), torch.empty_like(p)
    err = torch.empty(1, dtype=torch.float64, device=dev)
    errs = []
    for t, items in enumerate(plan, 1):
        if paired:
            lr = np.stack([_window(imgs[i][0], y0, x0, ch, cw, k) for i, y0, x0, k in items])
            hr = np.stack([_window(imgs[i][1], f * y0, f * x0, f * ch, f * cw, k) for i, y0, x0, k in items])
            eng.backprop_pair_dev(torch.from_numpy(lr).to(dev).contiguous(), torch.from_numpy(hr).to(dev).contiguous(), p, linear, None, l2,
                                  grad=g, err=err)
        else:
            hr = np.stack([_window(imgs[i], y0, x0, ch, cw, k) for i, y0, x0, k in items])
            eng.backprop_dev(torch.from_numpy(hr).to(dev).contiguous(), p, linear, None, l2, grad=g, err=err)
        eng.adam_step_dev(p, m, v, g, t)
        torch.cuda.synchronize()
        errs.append(float(err.item()))
    return np.array(errs), p.cpu().numpy()


def _session(eng, start, imgs, plan, ch, cw, linear, l2, store_bytes, resident=lambda i: True, paired=False):
    import rusty_sr_amd as r
    tr = r.Trainer(eng, start, linear_loss=linear, l2=l2, store_bytes=store_bytes)
    try:
        add = (lambda im: tr.add_pair(*im)) if paired else tr.add_image
        ids = [add(im) if resident(i) else -1 for i, im in enumerate(imgs)]
        for items in plan:
            its = [(ids[i] if ids[i] >= 0 else imgs[i], y0, x0, k) for i, y0, x0, k in items]
            (tr.step_pair_crops if paired else tr.step_crops)(its, ch, cw)
        return np.array(tr.sync()), tr.params(), ids
    finally:
        tr.close()


RESIDENCY = ((1 << 30, lambda i: True, lambda ids: min(ids) >= 0),                          # everything resident
             (0, lambda i: True, lambda ids: max(ids) == -1),                               # every image transient
             (1 << 30, lambda i: i % 2 == 0, lambda ids: ids[0] >= 0 and ids[1] == -1))     # every other image resident

# test_gpu_train.CASES, and one crop above 32 on both axes
CASES = [(2, 19, 23, False), (3, 24, 19, True), (4, 21, 26, False), (3, 35, 41, False)]


@pytest.mark.parametrize("f,ch,cw,linear", CASES)
def test_augmented_steps_equal_backprop_on_transformed_numpy_crops(f, ch, cw, linear):
    import rusty_sr_amd as r
    start = synthetic_params(f, 40 + f)
    imgs = _images(10 * f)
    plan = _plan(len(imgs), f, ch, cw)
    eng = r.Engine(start, device=0, factor=f)
    try:
        want = _reference(eng, start, imgs, plan, ch, cw, linear, 1e-6)
        for store, resident, check in RESIDENCY:
            got_err, got_p, ids = _session(eng, start, imgs, plan, ch, cw, linear, 1e-6, store, resident)
            assert check(ids), ids
            assert _bits_equal((got_err, got_p), want), (store, got_err, want[0])
    finally:
        eng.close()


PAIR_CASES = [(2, 9, 11, False), (3, 8, 7, True), (4, 5, 6, False), (3, 12, 35, False)]


@pytest.mark.parametrize("f,clh,clw,linear", PAIR_CASES)
def test_augmented_pair_steps_equal_pair_backprop_on_transformed_numpy_crops(f, clh, clw, linear):
    import rusty_sr_amd as r
    start = synthetic_params(f, 60 + f)
    pairs = _pair_images(f, 20 * f)  # LR / HR channel counts 3 and 4, mixed
    plan = _plan(len(pairs), 100 + f, clh, clw, lo=17)
    eng = r.Engine(start, device=0, factor=f)
    try:
        want = _reference(eng, start, pairs, plan, clh, clw, linear, 1e-6, paired=True)
        for store, resident, check in RESIDENCY:
            got_err, got_p, ids = _session(eng, start, pairs, plan, clh, clw, linear, 1e-6, store, resident, paired=True)
            assert check(ids), ids
            assert _bits_equal((got_err, got_p), want), (store, got_err, want[0])
    finally:
        eng.close()


# ---- the entry points themselves

def _raw_step(tr, items, members, ch, cw, paired=False):
    """sr_train_step_aug / sr_train_step_pairs_aug on resident ids, members a list or None (NULL) -> the status"""
    from rusty_sr_amd import _lib
    arr = ((_lib.TrainPairCrop if paired else _lib.TrainCrop) * len(items))()
    for it, (i, y0, x0) in zip(arr, items):
        it.y0, it.x0 = y0, x0
        if paired:
            it.pair = i
        else:
            it.image = i
    mem = None if members is None else (C.c_uint8 * len(members))(*members)
    fn = tr._L.sr_train_step_pairs_aug if paired else tr._L.sr_train_step_aug
    rc = fn(tr._t, arr, mem, len(items), ch, cw)
    if rc == _lib.SR_OK:
        tr.steps += 1
        tr._pending += 1
    return rc


@pytest.mark.parametrize("paired", [False, True])
def test_member_0_is_the_plain_call(paired):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    f, ch, cw = 3, (8 if paired else 24), (7 if paired else 19)
    start = synthetic_params(f, 71)
    imgs = _pair_images(f, 5) if paired else _images(5)
    plan = [[(i, y0, x0) for i, y0, x0, _ in items] for items in _plan(len(imgs), 9, ch, cw, lo=17 if paired else 50)]
    eng = r.Engine(start, device=0, factor=f)
    try:
        got = []
        for how in ("plain", "null", "zeros"):
            tr = r.Trainer(eng, start)
            ids = [tr.add_pair(*im) if paired else tr.add_image(im) for im in imgs]
            for items in plan:
                its = [(ids[i], y0, x0) for i, y0, x0 in items]
                if how == "plain":
                    (tr.step_pair_crops if paired else tr.step_crops)(its, ch, cw)
                else:
                    assert _raw_step(tr, its, None if how == "null" else [0] * len(its), ch, cw, paired) == _lib.SR_OK
            got.append((np.array(tr.sync()), tr.params()))
            tr.close()
        assert len(got[0][0]) == len(plan)
        assert _bits_equal(got[1], got[0]) and _bits_equal(got[2], got[0])
    finally:
        eng.close()


def test_every_member_changes_the_step():
    """a member that is parsed and then ignored would give member 0's parameters"""
    import rusty_sr_amd as r
    start = synthetic_params(3, 23)
    img = np.random.default_rng(8).integers(0, 256, (24, 24, 3), dtype=np.uint8)  # no symmetry
    eng = r.Engine(start, device=0, factor=3)
    try:
        seen = []
        for k in range(8):
            tr = r.Trainer(eng, start)
            tr.step_crops([(tr.add_image(img), 2, 3, k)], 18, 18)
            tr.sync()
            seen.append(tr.params().tobytes())
            tr.close()
        assert all(seen[k] != seen[0] for k in range(1, 8))
        assert len(set(seen)) == 8
    finally:
        eng.close()


def test_bad_members_are_refused_and_the_session_keeps_working():
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    start = synthetic_params(3, 11)
    img = synth_u8(5, 1, 20, 20)[0]
    lr = synth_u8(6, 1, 8, 8)[0]
    hr = synth_u8(7, 1, 24, 24)[0]
    eng = r.Engine(start, device=0, factor=3)
    try:
        def run(bad):
            tr = r.Trainer(eng, start)
            i, p = tr.add_image(img), tr.add_pair(lr, hr)
            if bad:
                for k in (8, 255):
                    assert _raw_step(tr, [(i, 0, 0), (i, 1, 1)], [3, k], 18, 18) == _lib.SR_E_INVALID
                    assert _raw_step(tr, [(p, 0, 0)], [k], 6, 6, paired=True) == _lib.SR_E_INVALID
                for k in (-1, 8):
                    with pytest.raises(ValueError):
                        tr.step_crops([(i, 0, 0, k)], 18, 18)
                    with pytest.raises(ValueError):
                        tr.step_pair_crops([(p, 0, 0, k)], 6, 6)
                assert tr.steps == 0
            tr.step_crops([(i, 0, 0, 5)], 18, 18)
            tr.step_pair_crops([(p, 1, 0, 6)], 6, 6)
            out = (np.array(tr.sync()), tr.params())
            tr.close()
            return out
        want, got = run(False), run(True)
        assert len(got[0]) == 2 and _bits_equal(got, want)  # nothing was launched by the refused calls
    finally:
        eng.close()


def test_augmented_steps_are_reproducible():
    import rusty_sr_amd as r
    f, clh, clw = 3, 8, 7
    start = synthetic_params(f, 31)
    pairs = _pair_images(f, 7)
    plan = _plan(len(pairs), 3, clh, clw, lo=17)

    def interleaved(eng):
        """plain, paired, augmented and un-augmented steps in one session"""
        tr = r.Trainer(eng, start)
        ids = [tr.add_pair(*pr) for pr in pairs]
        plain = [tr.add_image(pr[1]) for pr in pairs]
        for s, items in enumerate(plan + plan):
            aug = s % 4 < 2
            if s % 2:
                tr.step_pair_crops([(ids[i], y0, x0) + ((k,) if aug else ()) for i, y0, x0, k in items], clh, clw)
            else:
                tr.step_crops([(plain[i], f * y0, f * x0) + ((k,) if aug else ()) for i, y0, x0, k in items], f * clh, f * clw)
        out = (np.array(tr.sync()), tr.params())
        tr.close()
        return out

    eng = r.Engine(start, device=0, factor=f)
    try:
        a = _session(eng, start, pairs, plan, clh, clw, False, 1e-6, 1 << 30, paired=True)
        b = _session(eng, start, pairs, plan, clh, clw, False, 1e-6, 1 << 30, paired=True)
        assert _bits_equal(a[:2], b[:2])
        c, d = interleaved(eng), interleaved(eng)
        assert len(c[0]) == 2 * len(plan) and _bits_equal(c, d)
    finally:
        eng.close()


# ---- rusty_sr train --augment

M64 = (1 << 64) - 1


class SplitMix64:
    """the generator of the CLI's draws (main.cpp Rng)"""

    def __init__(self, seed):
        self.s = seed & M64

    def next(self):
        self.s = (self.s + 0x9e3779b97f4a7c15) & M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
        return z ^ (z >> 31)


def _cli_draws(sizes, seed, steps, unit, augment):
    """`rusty_sr train`'s draws, restated: files in path order; each epoch a Fisher-Yates shuffle of them (i = n .. 2: swap entry i - 1
    with entry next() % i); each draw the next file of the shuffle and a crop origin uniform over the positions inside the image (0 on an
    axis no longer than the crop), y0 then x0, all from the stream seeded with seed ^ 0x5eed5eed5eed5eed; with --augment each draw's
    member is next() >> 61 of a second stream seeded with seed ^ 0x6175676d656e7421.  Sizes and origins are in crop units (LR pixels
    for pairs: unit = f); the crop is 192 / unit; a step is 4 draws."""
    rng, aug = SplitMix64(seed ^ 0x5eed5eed5eed5eed), SplitMix64(seed ^ 0x6175676d656e7421)
    crop = 192 // unit
    perm, pos, out = [], 0, []
    for _ in range(4 * steps):
        if pos == len(perm):
            perm, pos = list(range(len(sizes))), 0
            for i in range(len(perm), 1, -1):
                j = rng.next() % i
                perm[i - 1], perm[j] = perm[j], perm[i - 1]
        fi = perm[pos]
        pos += 1
        h, w = sizes[fi][0] // unit, sizes[fi][1] // unit
        y0 = rng.next() % (h - crop + 1) if h > crop else 0
        x0 = rng.next() % (w - crop + 1) if w > crop else 0
        out.append((fi, y0, x0, aug.next() >> 61 if augment else 0))
    return [out[4 * s:4 * s + 4] for s in range(steps)]


def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _train(*args):
    res = subprocess.run([_cli(), "train", *args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    return res


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """hr: generated PNGs of 150 .. 330 pixels a side, one below 192 rows (even sizes); lr: their 2 x 2 byte means; flat: images of one
    colour each, larger than the crop"""
    from PIL import Image
    root = tmp_path_factory.mktemp("augment_cli")
    hr_dir, lr_dir, flat_dir = root / "hr", root / "lr", root / "flat"
    for d in (hr_dir, lr_dir, flat_dir):
        d.mkdir()
    hrs, lrs = [], []
    for k, (h, w) in enumerate([(256, 300), (210, 260), (150, 300), (300, 220), (200, 330)]):
        hr = synth_u8(170 + k, 1, h, w)[0]
        lr = (hr.reshape(h // 2, 2, w // 2, 2, 3).astype(np.int32).sum(axis=(1, 3)) // 4).astype(np.uint8)
        Image.fromarray(hr).save(hr_dir / f"t{k}.png")
        Image.fromarray(lr).save(lr_dir / f"t{k}.png")
        hrs.append(hr)
        lrs.append(lr)
    for k, (h, w) in enumerate([(200, 230), (192, 260), (250, 215), (230, 230)]):
        Image.fromarray(np.full((h, w, 3), (40 * k + 10, 200 - 30 * k, 17 * k + 3), np.uint8)).save(flat_dir / f"c{k}.png")
    return root, str(hr_dir), str(lr_dir), str(flat_dir), hrs, lrs


def test_cli_augmented_training_is_the_restated_draws(folders):
    import rusty_sr_amd as r
    root, hr_dir, _, _, hrs, _ = folders
    seed, steps = 21, 5
    out = str(root / "aug.rsr")
    _train("--augment", "--seed", str(seed), "--steps", str(steps), out, hr_dir)
    plan = _cli_draws([im.shape[:2] for im in hrs], seed, steps, 1, True)
    assert len({k for items in plan for *_, k in items}) >= 6  # (20 draws: the members are not all one value)
    start = r.init_params(3, seed)
    eng = r.Engine(start, device=0, factor=3)
    try:
        tr = r.Trainer(eng, start)
        ids = [tr.add_image(im) for im in hrs]
        for items in plan:
            tr.step_crops([(ids[i], y0, x0, k) for i, y0, x0, k in items], 192, 192)
        tr.sync()
        assert r.rsr.encode(tr.params()) == open(out, "rb").read()
        tr.close()
    finally:
        eng.close()


def test_cli_augmented_pair_training_is_the_restated_draws(folders):
    import rusty_sr_amd as r
    root, hr_dir, lr_dir, _, hrs, lrs = folders
    seed, steps = 22, 5
    out = str(root / "aug_pairs.rsr")
    _train("--augment", "--seed", str(seed), "--steps", str(steps), "-f", "2", "--lr_folder", lr_dir, out, hr_dir)
    plan = _cli_draws([im.shape[:2] for im in hrs], seed, steps, 2, True)
    start = r.init_params(2, seed)
    eng = r.Engine(start, device=0, factor=2)
    try:
        tr = r.Trainer(eng, start)
        ids = [tr.add_pair(lr, hr) for lr, hr in zip(lrs, hrs)]
        for items in plan:
            tr.step_pair_crops([(ids[i], y0, x0, k) for i, y0, x0, k in items], 96, 96)
        tr.sync()
        assert r.rsr.encode(tr.params()) == open(out, "rb").read()
        tr.close()
    finally:
        eng.close()


_BLOBS = {}


def _trained(root, folder, *flags, fresh=False):
    """the parameter file of `train [flags] --seed 33 --steps 3` on folder; each command runs once unless fresh"""
    key = (folder, flags)
    if fresh or key not in _BLOBS:
        out = str(root / f"run{len(_BLOBS)}{'f' if fresh else ''}.rsr")
        _train(*flags, "--seed", "33", "--steps", "3", out, folder)
        blob = open(out, "rb").read()
        if fresh:
            return blob
        _BLOBS[key] = blob
    return _BLOBS[key]


def test_cli_member_stream_leaves_shuffles_and_origins_alone(folders):
    """every transform of a crop of one colour is that crop: on such a folder --augment must change nothing, so the first stream's
    draws are those of a run without the flag; on real images the members do change the file"""
    root, hr_dir, _, flat_dir, _, _ = folders
    assert _trained(root, flat_dir, "--augment") == _trained(root, flat_dir)
    assert _trained(root, hr_dir, "--augment") != _trained(root, hr_dir)


def test_cli_augmented_training_is_repeatable(folders):
    root, hr_dir, _, _, _, _ = folders
    assert _trained(root, hr_dir, "--augment", fresh=True) == _trained(root, hr_dir, "--augment")
