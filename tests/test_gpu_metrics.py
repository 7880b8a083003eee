"""Y-channel PSNR and SSIM on the GPU (include/srhip.h "Metrics": sr_image_metrics_*, sr_pool_validation_metrics_*, sr_pair_validation_metrics_*) against the numpy
restatement tests/metrics_ref.py.  Every acceptance: y_sq_err, y_count, ssim_count equal as integers, and the per-image SSIM within
TOL of the restatement's -- 400 x the largest difference between two f64 evaluation orders of the map's mean (4.5e-13, separable against
direct 2-D), 1 / 38 000 of what an f32 filter misses by (3.8e-5 on a bright flat image): any f64 summation order passes, no f32 one."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
import torch

import metrics_ref as ref
from conftest import synth_u8
from ensemble_ref import quantise
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

TOL = 1e-9


def tile():
    from rusty_sr_amd import _lib
    return _lib.SR_METRICS_TILE


def noisy(img, seed, amp=6):
    rng = np.random.default_rng(seed)
    return np.clip(img.astype(np.int32) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def with_channels(img, ch, seed):
    if ch == 3:
        return np.ascontiguousarray(img[..., :3])
    alpha = np.random.default_rng(seed).integers(0, 256, img.shape[:2] + (1,), dtype=np.uint8)  # (must not matter)
    return np.concatenate([img[..., :3], alpha], axis=-1)


def at_offset(img, off):
    """The image in device memory, its first byte `off` bytes behind a 4-byte aligned address."""
    flat = torch.from_numpy(np.ascontiguousarray(img).reshape(-1))
    buf = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device="cuda")
    view = buf[off:off + flat.numel()]
    view.copy_(flat)
    t = view.view(img.shape)
    assert t.data_ptr() % 4 == off and t.is_contiguous()
    return t


def result_slot(fill=0xEE):
    """16 bytes at a 4-byte aligned address that is not 8-byte aligned."""
    buf = torch.full((32,), fill, dtype=torch.uint8, device="cuda")
    out = buf[4:20]
    assert out.data_ptr() % 8 == 4
    return buf, out


def accept(got, want, where=""):
    for k in ("y_sq_err", "y_count", "ssim_count"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    if want["ssim_count"] == 0:
        assert got["ssim_sum"] == 0.0 and not math.copysign(1, got["ssim_sum"]) < 0, (where, got["ssim_sum"])
    else:
        diff = abs(got["ssim_sum"] / got["ssim_count"] - want["ssim"])
        assert diff <= TOL, (where, diff, got["ssim_sum"] / got["ssim_count"], want["ssim"])


@pytest.fixture(scope="module")
def eng(params):
    import rusty_sr_amd as r
    e = r.Engine(params["imagenet"], device=0)
    yield e
    e.close()


def dev_metrics(e, a, b, shave, off_a=0, off_b=0):
    import rusty_sr_amd as r
    buf, out = result_slot()
    e.image_metrics_dev(at_offset(a, off_a), at_offset(b, off_b), shave=shave, out=out)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:4] == 0xEE) and np.all(host[20:] == 0xEE)  # nothing but the 16 bytes is written
    return r.metrics_from_bytes(host[4:20], a.shape[0], a.shape[1], shave)


def boundary_sizes():
    T = tile()
    d = [T + 9, T + 10, T + 11, 2 * T + 10, 2 * T + 11, T, T + 1, 2 * T, 2 * T + 1]  # windows, then pixels, either side of a tile
    out = [(11, 11), (10, 40), (40, 10)]
    for i, h in enumerate(d):
        out += [(h, d[(2 * i + 1) % len(d)]), (d[(2 * i + 3) % len(d)], h)]
    return out


def random_sizes():
    rng = np.random.default_rng(2024)
    return [tuple(int(v) for v in rng.integers(9, 101, 2)) for _ in range(30)]


def test_kernel_at_tile_boundaries_and_random_sizes(eng):
    """image_metrics_dev alone: sizes either side of every tile boundary at shave 0, then 30 random sizes; shaves 0, 2, 3, 4; 3 or 4
    channels per operand; both pointers at every byte offset; the result at a 4-byte aligned address that is not 8-byte aligned."""
    rng = np.random.default_rng(7)
    cases = [(h, w, 0) for h, w in boundary_sizes()] + [(h, w, (0, 2, 3, 4)[i % 4]) for i, (h, w) in enumerate(random_sizes())]
    seen_off = set()
    for i, (h, w, s) in enumerate(cases):
        base = synth_u8(100 + i, 1, h, w)[0]
        ca, cb, oa, ob = (3, 4)[i % 2], (3, 4)[(i // 2) % 2], i % 4, int(rng.integers(0, 4))
        a, b = with_channels(noisy(base, 200 + i), ca, i), with_channels(base, cb, i + 1)
        seen_off.add((oa, ob))
        accept(dev_metrics(eng, a, b, s, oa, ob), ref.metrics(a, b, s), (h, w, s, ca, cb, oa, ob))
    assert {o for o, _ in seen_off} == {0, 1, 2, 3} == {o for _, o in seen_off}


@pytest.mark.parametrize("h,w", [(45, 70), (43, 33)])
@pytest.mark.parametrize("shave", [0, 3])
def test_kernel_arithmetic_stress(eng, h, w, shave):
    white, black = np.full((h, w, 3), 255, np.uint8), np.zeros((h, w, 3), np.uint8)
    board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)[..., None].repeat(3, axis=2)
    img = synth_u8(9, 1, h, w)[0]
    for name, a, b in (("bright flat against its noisy copy", noisy(white, 1), white), ("black against white", black, white),
                       ("checkerboard against its inverse", board, 255 - board)):
        got = dev_metrics(eng, a, b, shave, 1, 2)
        accept(got, ref.metrics(a, b, shave), name)
    for a in (img, white, board):  # identical operands: exactly one per window, zero error
        got = dev_metrics(eng, a, a.copy(), shave, 3, 0)
        assert got["y_sq_err"] == 0 and got["ssim_sum"] == got["ssim_count"] == (h - 2 * shave - 10) * (w - 2 * shave - 10)


def test_degenerate_regions(eng):
    from rusty_sr_amd import _lib
    zero = {"y_sq_err": 0, "y_count": 0, "ssim_sum": 0.0, "ssim_count": 0}
    for h, w, s in ((6, 30, 3), (30, 8, 4), (5, 5, 3), (1, 1, 1)):   # nothing left: all four fields zero, SR_OK, the 16 bytes written
        a = synth_u8(h + w, 1, h, w)[0]
        got = dev_metrics(eng, a, noisy(a, 3), s)
        assert {k: got[k] for k in zero} == zero
        assert eng.image_metrics(a, noisy(a, 3), shave=s)["y_count"] == 0
    for side in range(11, 21):   # a shaved side below 11: the Y sums set, no window; from 11 on the windows of the definition
        for s in (3, 4):
            for h, w in ((side, 40), (40, side)):
                a = synth_u8(side, 1, h, w)[0]
                b = noisy(a, side + s)
                want = ref.metrics(a, b, s)
                assert want["y_count"] > 0 and (want["ssim_count"] == 0) == (side - 2 * s < 11)
                accept(dev_metrics(eng, a, b, s), want, (h, w, s))
                host = eng.image_metrics(a, b, shave=s)
                accept(host, want, (h, w, s, "host"))
                assert host["y_psnr"] == want["y_psnr"] and (host["ssim"] is None) == (want["ssim"] is None)
    # refusals: nothing is launched, the result stays untouched
    a = synth_u8(1, 1, 20, 20)[0]
    da, (buf, out) = at_offset(a, 0), result_slot()
    L, ctx, vp = eng._L, eng._ctx, C.c_void_p
    assert L.sr_image_metrics_rgba8_dev(ctx, vp(da.data_ptr()), 3, vp(da.data_ptr()), 3, 20, 20, -2, vp(out.data_ptr()), None) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8_dev(ctx, None, 3, vp(da.data_ptr()), 3, 20, 20, 0, vp(out.data_ptr()), None) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8_dev(ctx, vp(da.data_ptr()), 3, None, 3, 20, 20, 0, vp(out.data_ptr()), None) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8_dev(ctx, vp(da.data_ptr()), 3, vp(da.data_ptr()), 3, 20, 20, 0, None, None) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8_dev(ctx, vp(da.data_ptr()), 3, vp(da.data_ptr()), 3, 20, 20, 0, vp(out.data_ptr() + 1), None) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8_dev(ctx, vp(da.data_ptr()), 5, vp(da.data_ptr()), 3, 20, 20, 0, vp(out.data_ptr()), None) == _lib.SR_E_INVALID
    m = _lib.Metrics()
    u8p = C.POINTER(C.c_uint8)
    assert L.sr_image_metrics_rgba8(ctx, a.ctypes.data_as(u8p), 3, a.ctypes.data_as(u8p), 3, 20, 20, -2, C.byref(m)) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8(ctx, None, 3, a.ctypes.data_as(u8p), 3, 20, 20, 0, C.byref(m)) == _lib.SR_E_INVALID
    assert L.sr_image_metrics_rgba8(ctx, a.ctypes.data_as(u8p), 3, a.ctypes.data_as(u8p), 3, 20, 20, 0, None) == _lib.SR_E_INVALID
    err, n = C.c_double(), C.c_size_t()
    assert L.sr_pool_validation_metrics_rgba8(ctx, a.ctypes.data_as(u8p), 3, 20, 20, 0, 0, -2, C.byref(err), C.byref(n), C.byref(m)) == _lib.SR_E_INVALID
    torch.cuda.synchronize()
    assert np.all(buf.cpu().numpy() == 0xEE)
    # shave -1 / None is the context's factor
    assert eng.image_metrics(a, noisy(a, 1)) == eng.image_metrics(a, noisy(a, 1), shave=3)


def test_any_graph_scores_images():
    """No network runs: a bilinear context scores two images like an sr_net one."""
    import rusty_sr_amd as r
    e = r.bilinear_net()
    a = synth_u8(4, 1, 40, 52)[0]
    b = noisy(a, 2)
    accept(e.image_metrics(a, b), ref.metrics(a, b, 3))
    e.close()


# ---- the validation calls ---------------------------------------------------------------------------------------------------------------
def saturated(h, w, seed):
    """Smooth noise with saturated black and white blocks beside each other: the network overshoots below 0 and above 1 at their edges."""
    img = synth_u8(seed, 1, h, w)[0].copy()
    img[: h // 3, : w // 2] = 0
    img[: h // 3, w // 2:] = 255
    img[h // 2:, w // 3: w // 3 + 6] = 255
    img[h // 2:, w // 3 + 6: w // 3 + 12] = 0
    return img


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision="f32"):
        k = (factor, precision)
        if k not in made:
            p = params["imagenet"] if factor == 3 else synthetic_params(factor, 100 + factor)
            made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def want_of_output(e, hr, shave):
    """The restatement on quantise(the GPU's own f32 output) against the HR crop the loss uses."""
    f = e.factor
    h, w = hr.shape[:2]
    _, out = e.validation_nodes(h, w)
    crop = hr[: f * (h // f), : f * (w // f)]
    return ref.metrics(quantise(out), crop, f if shave is None else shave), out


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
@pytest.mark.parametrize("f", [2, 3, 4])
def test_validation_metrics(engines, f, precision):
    """Pooled and paired, linear_loss 0 / 1, plain and ensemble of 8, host and device forms: err_sum and n_elems are the bits of the existing
    call on the same input, the scores those of the restatement on quantise(output)."""
    import rusty_sr_amd as r
    e = engines(f, precision)
    clamped = False
    for (h, w), ch in (((48, 60), 3), ((50, 47), 4)):   # (50 x 47: the crop rule, at every factor)
        hr = with_channels(saturated(h, w, 10 * f + h), ch, 5)
        lr = with_channels(synth_u8(20 * f + h, 1, h // f, w // f)[0], 7 - ch, 6)
        hr_pair = np.ascontiguousarray(hr[: f * (h // f), : f * (w // f)])
        for linear in (False, True):
            for members in (None, r._lib.SR_ENSEMBLE_ALL):
                for shave in (None, 0):
                    got = e.validation_metrics(hr, linear_loss=linear, members=members, shave=shave)
                    want, out = want_of_output(e, hr, shave)
                    clamped |= bool(out.min() < 0 and out.max() > 1)
                    accept(got, want, (f, precision, h, w, linear, members, shave, "pooled"))
                    assert (got["err_sum"], got["n_elems"]) == e.validation_error(hr, linear, members=members)
                    assert got["y_psnr"] == want["y_psnr"]
                got = e.validation_metrics(hr_pair, lr=lr, linear_loss=linear, members=members)
                want, _ = want_of_output(e, hr_pair, None)
                accept(got, want, (f, precision, h, w, linear, members, "paired"))
                assert (got["err_sum"], got["n_elems"]) == e.validation_error_pair(lr, hr_pair, linear, members=members)
            # the device forms (no ensemble), result at a 4-byte aligned address, images at odd bytes
            for pair in (False, True):
                b, d_hr = (hr_pair, at_offset(hr_pair, 1)) if pair else (hr, at_offset(hr, 3))
                d_lr = at_offset(lr, 2) if pair else None
                buf, out16 = result_slot()
                err = torch.zeros(1, dtype=torch.float64, device="cuda")
                e.validation_metrics_dev(d_hr, lr=d_lr, linear_loss=linear, shave=2, err=err, out=out16)
                torch.cuda.synchronize()
                want, _ = want_of_output(e, b, 2)
                HC, WC = f * (b.shape[0] // f), f * (b.shape[1] // f)
                accept(r.metrics_from_bytes(buf.cpu().numpy()[4:20], HC, WC, 2), want, (f, precision, h, w, linear, pair, "dev"))
                plain = e.validation_error_pair_dev(d_lr, d_hr, linear) if pair else e.validation_error_dev(d_hr, linear)
                torch.cuda.synchronize()
                assert err.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes()
    if f == 3:
        assert clamped, "no output below 0 and above 1: the clamp of the quantisation was not exercised"


def test_same_bits_on_every_run_and_context(eng, params):
    import rusty_sr_amd as r
    a = synth_u8(31, 1, 90, 77)[0]
    b = noisy(a, 8)
    da, db = at_offset(a, 0), at_offset(b, 0)
    other = r.Engine(params["imagenet"], device=0)
    runs = []
    for e in (eng, eng, other):
        out = e.image_metrics_dev(da, db, shave=2)
        torch.cuda.synchronize()
        runs.append(out.cpu().numpy().tobytes())
    hr = saturated(48, 60, 3)
    vals = [e.validation_metrics(hr) for e in (eng, eng, other)]
    other.close()
    assert runs[0] == runs[1] == runs[2]
    assert vals[0] == vals[1] == vals[2]


def test_metrics_leave_no_trace_on_the_plain_path(eng):
    hr = saturated(50, 47, 4)
    before = eng.validation_error(hr)
    eng.validation_metrics(hr, members=0x0F, shave=1)
    eng.image_metrics(hr, noisy(hr, 1))
    assert eng.validation_error(hr) == before


# ---- the aggregate and the CLI ---------------------------------------------------------------------------------------------------------
def test_python_aggregate_and_cli(tmp_path, params):
    from PIL import Image
    from rusty_sr_amd.build import build_host
    import rusty_sr_amd as r
    cli = build_host()
    folder = tmp_path / "val"
    folder.mkdir()
    imgs = [saturated(48, 60, 1), synth_u8(2, 1, 12, 14)[0], synth_u8(3, 1, 50, 47)[0]]  # b.png: too small for a window at shave 3
    for name, img in zip("abc", imgs):
        Image.fromarray(img).save(folder / (name + ".png"))
    e = r.Engine(params["anime"], device=0)
    got = r.validation_metrics([e], imgs)
    per = []
    for img, g in zip(imgs, got["per_image"]):
        e.validation_metrics(img)
        want, _ = want_of_output(e, img, None)
        accept(g, want)
        per.append(dict(want, err_sum=g["err_sum"], n_elems=g["n_elems"]))
    want = ref.aggregate(per)
    assert got["skipped"] == want["skipped"] == [(1, "ssim")]
    assert got["psnr"] == r.validation_psnr([e], imgs) and got["y_psnr"] == pytest.approx(want["y_psnr"], abs=1e-12)
    assert abs(got["ssim"] - want["ssim"]) <= TOL
    got8 = r.validation_metrics(e, imgs, members=r._lib.SR_ENSEMBLE_ALL, shave=0)
    assert got8["psnr"] == r.validation_psnr([e], imgs, members=r._lib.SR_ENSEMBLE_ALL) and got8["skipped"] == []
    e.close()

    def run(*args):
        res = subprocess.run([cli, "validate", "-p", "anime", *args, str(folder)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        return res.stdout.splitlines(), res.stderr
    plain, plain_err = run()
    lines, err = run("--metrics")
    assert len(plain) == 2 and plain[1].startswith("Validation PSNR:\t") and plain_err == ""
    assert lines[:2] == plain and len(lines) == 4
    assert lines[2].startswith("Y-PSNR:\t") and lines[3].startswith("SSIM:\t")
    assert np.float32(lines[1].split("\t")[1]) == np.float32(got["psnr"])
    assert np.float32(lines[2].split("\t")[1]) == np.float32(got["y_psnr"])
    assert np.float32(lines[3].split("\t")[1]) == np.float32(got["ssim"])
    assert "b.png" in err and "SSIM" in err and "a.png" not in err and "c.png" not in err
    lines0, err0 = run("--metrics", "--shave", "0", "--ensemble", "8")
    assert np.float32(lines0[2].split("\t")[1]) == np.float32(got8["y_psnr"]) and np.float32(lines0[3].split("\t")[1]) == np.float32(got8["ssim"])
    assert err0 == ""
