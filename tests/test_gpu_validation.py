"""The validation pass on the GPU (include/srhip.h sr_validation_error_*; reference main.rs:220-247, network.rs:88-102) against an f64
restatement in this file: the pool (anchored on oracle.downsample at factor 3), the network (oracle.forward_factor, f64), the loss."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, load_png, synth_u8
from param_families import bundled_scale as synthetic_params   # (the one generator of bundled-scale weights)

pytestmark = pytest.mark.gpu

POOL_TOL = 2e-6   # the pool's stated error (sr_valid.hip): hardware log2 / exp2 transfer functions, f32 sums
GOLDENS = ("cartoon_rsa.png", "butterfly_rs.png", "logo_nn.png")
F32_0_04045 = np.float32(0.04045)


# ---- the f64 restatement -----------------------------------------------------------------------------------------------------
def hr_values(hr):
    """img_to_data (byte / 255 in f32, alpha dropped) or the f32 image as is, as f32."""
    return hr[..., :3].astype(np.float32) / np.float32(255) if hr.dtype == np.uint8 else hr.astype(np.float32)


def s2l(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(x <= np.float64(F32_0_04045), x / 12.92, ((np.maximum(x, 0.04) + 0.055) / 1.055) ** 2.4)


def l2s(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.maximum(v, 0.0031) ** (1 / 2.4) - 0.055)


def pool64(hr, f):
    x = hr_values(hr).astype(np.float64)
    oh, ow = x.shape[0] // f, x.shape[1] // f
    lin = s2l(x[:f * oh, :f * ow]).reshape(oh, f, ow, f, 3)
    return l2s(lin.mean(axis=(1, 3)))


def crop(hr, f):
    return hr_values(hr)[:f * (hr.shape[0] // f), :f * (hr.shape[1] // f)]


def err_of(out32, hr, f, linear):
    """The loss as the GPU defines it: each difference in f32, squares summed in f64 (linear: of the correctly rounded f32
    SrgbToLinear of both sides)."""
    h = crop(hr, f)
    if linear:
        d = s2l(out32).astype(np.float32) - s2l(h).astype(np.float32)
    else:
        d = out32.astype(np.float32) - h
    d = d.astype(np.float64).ravel()
    return math.fsum(d * d), d.size


def psnr(err, n):
    return math.inf if err == 0 else -10 * math.log10(err / n)


_oracle_cache = {}


def oracle_psnr(key, p, hr, f, linear):
    """-10 log10 of the f64 loss of the f64 network on the f64 pool."""
    k = (key, f, linear)
    if k not in _oracle_cache:
        out = oracle.forward_factor(p, pool64(hr, f)[None], f, f64=True)[0]
        h = crop(hr, f).astype(np.float64)
        d = (s2l(out) - s2l(h)) if linear else (out - h)
        _oracle_cache[k] = psnr(float(np.sum(d * d)), d.size)
    return _oracle_cache[k]


def hr_image(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "u8_3":
        return synth_u8(seed, 1, h, w)[0]
    if kind == "u8_4":
        return np.concatenate([synth_u8(seed, 1, h, w)[0], rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
    return rng.random((h, w, 3), dtype=np.float32)


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision="f32", key="imagenet"):
        k = (factor, precision, key)
        if k not in made:
            p = params[key] if factor == 3 else synthetic_params(factor, 100 + factor)
            made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def test_restatement_pool_is_the_downsample_oracle():
    x = oracle.img_to_data(synth_u8(5, 1, 31, 40))
    np.testing.assert_allclose(pool64(x[0], 3), oracle.downsample(x, f64=True)[0], rtol=0, atol=1e-12)


@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("kind", ["u8_3", "u8_4", "f32"])
def test_pool_matches_restatement(engines, f, kind):
    e = engines(f)
    shapes = [(96, 96), (100, 77), (f, f)] + ([(7, 5)] if f == 4 else [])
    for i, (h, w) in enumerate(shapes):
        hr = hr_image(kind, h, w, 10 * f + i)
        err, n = e.validation_error(hr)
        assert n == 3 * f * (h // f) * f * (w // f)
        lr, out = e.validation_nodes(h, w)
        want = pool64(hr, f)
        assert lr.shape == want.shape and out.shape == (f * (h // f), f * (w // f), 3)
        assert float(np.abs(lr - want).max()) <= POOL_TOL, (h, w)
        assert err == pytest.approx(err_of(out, hr, f, False)[0], rel=1e-12)


@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("linear", [False, True])
def test_reduction_is_exact(engines, f, linear):
    e = engines(f)
    for kind, (h, w) in (("u8_4", (97, 130)), ("u8_3", (64, 64)), ("f32", (50, 71))):
        hr = hr_image(kind, h, w, 7 * f + h)
        err, n = e.validation_error(hr, linear_loss=linear)
        _, out = e.validation_nodes(h, w)
        want, m = err_of(out, hr, f, linear)
        assert n == m
        assert err == pytest.approx(want, rel=1e-12), (kind, err, want)


def test_refusals(engines, params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e = engines(3)
    for hr in (np.zeros((2, 9, 3), np.uint8), np.zeros((9, 2, 4), np.uint8), np.zeros((2, 2, 3), np.float32)):
        with pytest.raises(r.SrError) as ex:
            e.validation_error(hr)
        assert ex.value.status == _lib.SR_E_INVALID
    L = _lib.lib()
    err, n = C.c_double(), C.c_size_t()
    px = np.zeros((9, 9, 4), np.uint8)
    assert L.sr_validation_error_rgba8(e._ctx, px.ctypes.data_as(C.POINTER(C.c_uint8)), 5, 9, 9, 0, C.byref(err), C.byref(n)) == _lib.SR_E_INVALID
    assert L.sr_validation_error_rgba8(e._ctx, px.ctypes.data_as(C.POINTER(C.c_uint8)), 4, 9, 9, 0, None, C.byref(n)) == _lib.SR_E_INVALID
    bl = r.bilinear_net()
    with pytest.raises(r.SrError) as ex:
        bl.validation_error(px)
    assert ex.value.status == _lib.SR_E_INVALID
    fresh = r.Engine(params["imagenet"])
    with pytest.raises(r.SrError):  # no validation call yet: no nodes
        fresh.validation_nodes(9, 9)
    fresh.close()


def _cases(params):
    hr_synth = synth_u8(41, 1, 120, 150)[0]
    cases = [(name, 3, params[name], img) for name in ("imagenet", "imagenetlinear", "anime")
             for img in GOLDENS + ("synth",)]
    cases += [("synthetic2", 2, synthetic_params(2, 102), "synth"), ("synthetic4", 4, synthetic_params(4, 104), "synth")]
    return hr_synth, cases


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_psnr_end_to_end(params, precision):
    import rusty_sr_amd as r
    hr_synth, cases = _cases(params)
    made = {}
    for key, f, p, img in cases:
        if (key, f) not in made:
            made[(key, f)] = r.Engine(p, factor=f, precision=precision)
        e = made[(key, f)]
        hr = hr_synth if img == "synth" else load_png(img)
        for linear in ((False, True) if key == "imagenetlinear" else (False,)):
            got = r.validation_psnr([e], [hr], linear_loss=linear)
            want = oracle_psnr((key, img), p, hr, f, linear)
            assert abs(got - want) <= 0.005, (key, img, linear, got, want)
            assert math.isfinite(got), got
    for e in made.values():
        e.close()


def test_deterministic_and_engine_count_free(params):
    import rusty_sr_amd as r
    imgs = [load_png(n) for n in GOLDENS] + [synth_u8(3, 1, 90, 120)[0]]
    a = r.Engine(params["anime"])
    first = [a.validation_error(x) for x in imgs]
    again = [a.validation_error(x) for x in imgs]
    assert first == again  # bit-identical floats
    b = r.Engine(params["anime"])
    one = r.validation_psnr([a], imgs)
    two = r.validation_psnr([a, b], imgs)
    assert one == two
    err = sum(e for e, _ in first)
    n = sum(m for _, m in first)
    assert one == -10 * math.log10(err / n)
    a.close(); b.close()


@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_dev_matches_host_and_leaves_upscale_alone(params, precision):
    import torch
    import rusty_sr_amd as r
    e = r.Engine(params["imagenet"], precision=precision)
    px = synth_u8(9, 1, 60, 83)
    before = e.upscale_rgba8(px)
    rgb = load_png("cartoon_rsa.png")[..., :3]
    hr = np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 7, np.uint8)], axis=-1)[:-2, :-1]  # sizes not divisible by 3
    hr = np.ascontiguousarray(hr)
    for linear in (False, True):
        err, _ = e.validation_error(hr, linear_loss=linear)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            d_hr = torch.from_numpy(hr).cuda()
            out = e.validation_error_dev(d_hr, linear_loss=linear, stream=s)
        s.synchronize()
        assert out.item() == err
    # a u8 image that starts at an odd byte of its allocation
    big = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), hr.ravel()])).cuda()
    view = big[3:].view(hr.shape)
    out = e.validation_error_dev(view)
    torch.cuda.synchronize()
    assert out.item() == e.validation_error(hr)[0]
    after = e.upscale_rgba8(px)
    np.testing.assert_array_equal(before, after)
    e.close()


def test_cli_validate_end_to_end(tmp_path, params):
    from PIL import Image
    from rusty_sr_amd.build import PNGLIB, build_host
    import rusty_sr_amd as r
    cli = build_host()
    folder = tmp_path / "val"
    (folder / "sub").mkdir(parents=True)
    for n in GOLDENS:
        (folder / n).write_bytes(open(os.path.join(GOLDEN, n), "rb").read())
    Image.fromarray(synth_u8(12, 1, 71, 100)[0]).save(folder / "odd_size.png")
    Image.fromarray(synth_u8(13, 1, 96, 120)[0]).save(folder / "photo.JPG", quality=90)
    Image.fromarray(synth_u8(14, 1, 60, 66)[0]).save(folder / "sub" / "deep.png")
    (folder / "readme.txt").write_text("not an image")

    L = C.CDLL(PNGLIB)
    L.srpng_decode_any_rgba8.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint8))]
    L.srpng_free.argtypes = [C.POINTER(C.c_uint8)]

    def decode(path):  # the CLI's own decoders: the API must see the pixels the CLI scores
        w, h, p = C.c_int(), C.c_int(), C.POINTER(C.c_uint8)()
        assert L.srpng_decode_any_rgba8(str(path).encode(), C.byref(w), C.byref(h), C.byref(p)) == 0, path
        a = np.ctypeslib.as_array(p, shape=(h.value, w.value, 4)).copy()
        L.srpng_free(p)
        return a

    top = sorted(str(p) for p in folder.iterdir() if p.suffix.lower() in (".png", ".jpg"))
    deep = sorted(top + [str(folder / "sub" / "deep.png")])
    e = r.Engine(params["anime"])

    def run(*args):
        res = subprocess.run([cli, "validate", *args], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.splitlines()
        assert lines[0].startswith("Validating using anime neural net parameters...")
        assert lines[-1].startswith("Validation PSNR:\t")
        return np.float32(lines[-1].split("\t")[1])  # the f32 the reference prints, in shortest round-trip digits

    imgs = [decode(p) for p in top]
    v = run("-p", "anime", str(folder))
    assert v == np.float32(r.validation_psnr([e], imgs))
    v_l = run("-p", "anime", "-l", str(folder))
    assert v_l != v and v_l == np.float32(r.validation_psnr([e], imgs, linear_loss=True))
    v2 = run("-p", "anime", "-m", "2", str(folder))
    assert v2 == np.float32(r.validation_psnr([e], imgs[:2]))
    vr = run("-p", "anime", "-r", "--timing", str(folder))
    assert vr == np.float32(r.validation_psnr([e], [decode(p) for p in deep]))
    # an undecodable image file: exit 1, named
    (folder / "broken.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\x00" * 20)
    res = subprocess.run([cli, "validate", "-p", "anime", str(folder)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 1 and "broken.png" in res.stderr
    e.close()
