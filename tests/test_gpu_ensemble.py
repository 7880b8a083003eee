"""The self-ensemble on the GPU (include/srhip.h sr_upscale_ensemble_*): each member against the plain call of the transformed image, masks
against the numpy accumulation of the plain calls' outputs (tests/ensemble_ref.py), both bit for bit; then the oracle, the validation
pass, what it buys in PSNR, the refusals and the state it leaves behind."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle
from conftest import load_png, synth_u8
from ensemble_ref import T, T_inv, accumulate, ensemble, members_of, quantise
from test_gpu_validation import crop, err_of, pool64, synthetic_params

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the project's parity bar, pre-quantisation f32 (tests/test_gpu_parity.py)
SHAPES = [(1, 1), (1, 5), (5, 1), (37, 129), (40, 70), (256, 256)]
MASKS = (0xFF, 0x0F, 0x03, 0xA5, 0x07)
PRECISIONS = ("f32", "split_f16")


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(precision="f32", key="imagenet", factor=3):
        k = (precision, key, factor)
        if k not in made:
            p = params[key] if factor == 3 else synthetic_params(factor, 100 + factor)
            made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def image_u8(seed, h, w, channels=3):
    px = synth_u8(seed, 1, h, w)[0]
    if channels == 4:
        px = np.concatenate([px, np.random.default_rng(seed).integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=-1)
    return px


# ---- 1. each member alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_each_member_alone_is_the_plain_call_of_the_transformed_image(engines, precision, h, w):
    e = engines(precision)
    px3, px4 = image_u8(h * 1000 + w, h, w), image_u8(h * 1000 + w + 1, h, w, 4)
    x = oracle.img_to_data(px3)
    for k in range(8):
        np.testing.assert_array_equal(e.upscale_ensemble_f32(x, members=1 << k), T_inv(e.upscale_f32(T(x, k)), k), err_msg=f"f32 member {k}")
        for px in (px3, px4):
            np.testing.assert_array_equal(e.upscale_ensemble_rgba8(px, members=1 << k), T_inv(e.upscale_rgba8(T(px, k)), k),
                                          err_msg=f"u8 x{px.shape[2]} member {k}")
    np.testing.assert_array_equal(e.upscale_ensemble_f32(x, members=1).view(np.uint32), e.upscale_f32(x).view(np.uint32))
    np.testing.assert_array_equal(e.upscale_ensemble_rgba8(px4, members=1), e.upscale_rgba8(px4))


@pytest.mark.parametrize("factor", [2, 4])
def test_each_member_alone_at_other_factors(engines, factor):
    e = engines("f32", factor=factor)
    h, w = 37, 129
    px = image_u8(factor, h, w, 4)
    x = oracle.img_to_data(px)
    for k in range(8):
        got = e.upscale_ensemble_f32(x, members=1 << k)
        assert got.shape == (factor * h, factor * w, 3)
        np.testing.assert_array_equal(got, T_inv(e.upscale_f32(T(x, k)), k), err_msg=f"member {k}")
        np.testing.assert_array_equal(e.upscale_ensemble_rgba8(px, members=1 << k), T_inv(e.upscale_rgba8(T(px, k)), k), err_msg=f"member {k}")


# ---- 2. masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_masks_are_the_ordered_f32_sum_of_the_plain_calls(engines, precision, h, w):
    import torch
    e = engines(precision)
    px = image_u8(7 * h + w, h, w)
    x = oracle.img_to_data(px)
    plain = {k: T_inv(e.upscale_f32(T(x, k)), k) for k in range(8)}
    for m in MASKS:
        ks = members_of(m)
        want = accumulate([plain[k] for k in ks], len(ks))
        got = e.upscale_ensemble_f32(x, members=m)
        np.testing.assert_array_equal(got, want, err_msg=f"mask {m:#x}")
        dev = e.upscale_ensemble_f32_dev(torch.from_numpy(x[None]).cuda(), members=m)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dev.cpu().numpy()[0], got, err_msg=f"dev, mask {m:#x}")
        # the RGBA8 form quantises that same f32 value once, at the end
        got8 = e.upscale_ensemble_rgba8(px, members=m)
        np.testing.assert_array_equal(got8, quantise(want), err_msg=f"u8, mask {m:#x}")
        dev8 = e.upscale_ensemble_rgba8_dev(torch.from_numpy(px[None]).cuda(), members=m)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dev8.cpu().numpy()[0], got8, err_msg=f"u8 dev, mask {m:#x}")


def test_a_batch_is_its_images_one_after_another(engines):
    e = engines("f32")
    px = synth_u8(77, 3, 19, 45)
    x = oracle.img_to_data(px)
    got, got8 = e.upscale_ensemble_f32(x, members=0xA5), e.upscale_ensemble_rgba8(px, members=0xFF)
    assert got.shape == (3, 57, 135, 3) and got8.shape == (3, 57, 135, 4)
    for i in range(3):
        np.testing.assert_array_equal(got[i], e.upscale_ensemble_f32(x[i], members=0xA5))
        np.testing.assert_array_equal(got8[i], e.upscale_ensemble_rgba8(px[i], members=0xFF))


# ---- 3. oracle parity --------------------------------------------------------------------------------------------------------
def check_u8(got, v_ref):
    """The rule of tests/test_gpu_parity.py: off by one at most, only at rounding knife-edges, on fewer than 1e-3 of the bytes."""
    want = oracle.data_to_rgba8(v_ref.astype(np.float32))
    assert got.shape == want.shape and (got[..., 3] == 255).all()
    d = got[..., :3].astype(int) - want[..., :3].astype(int)
    assert np.abs(d).max() <= 1
    if (d != 0).any():
        frac = 255.0 * v_ref.astype(np.float64) + 0.5
        edge = np.abs(frac - np.round(frac))
        assert edge[d != 0].max() < 255 * TOL, "u8 mismatch away from a rounding knife-edge"
        assert (d != 0).mean() < 1e-3


def oracle_ensemble64(p, x, members=0xFF):
    ks = members_of(members)
    return np.mean([T_inv(oracle.forward(p, T(x, k).astype(np.float64), f64=True)[0], k) for k in ks], axis=0)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("source", ["synth", "cartoon_lr.png"])
def test_oracle_parity(engines, params, precision, source):
    key = "imagenet" if source == "synth" else "anime"
    e = engines(precision, key)
    px = image_u8(31, 40, 70) if source == "synth" else np.ascontiguousarray(load_png(source)[..., :3])
    x = oracle.img_to_data(px)
    want = oracle_ensemble64(params[key], x)
    got = e.upscale_ensemble_f32(x, members=0xFF)
    dev = float(np.abs(got.astype(np.float64) - want).max())
    print(f"[ensemble parity] {source} {precision}: max |gpu - oracle| = {dev:.3e}")
    assert dev < TOL
    check_u8(e.upscale_ensemble_rgba8(px, members=0xFF), want)


# ---- 4. validation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_validation_scores_the_ensemble_output(engines, precision):
    e = engines(precision)
    for i, (h, w, ch) in enumerate([(96, 96, 3), (100, 77, 4), (3, 3, 3)]):
        hr = image_u8(500 + i, h, w, ch)
        plain_err, plain_n = e.validation_error(hr)
        lr_plain, _ = e.validation_nodes(h, w)
        err, n = e.validation_error(hr, members=0xFF)
        assert n == plain_n == 3 * 3 * (h // 3) * 3 * (w // 3)
        lr, out = e.validation_nodes(h, w)
        np.testing.assert_array_equal(lr, lr_plain)
        # `output` is the ensemble of the plain calls on the `input` node the pass reports
        np.testing.assert_array_equal(out, ensemble(lambda t: e.upscale_f32(t), lr, 0xFF))
        assert err == pytest.approx(err_of(out, hr, 3, False)[0], rel=1e-12)  # (the bound of tests/test_gpu_validation.py for this comparison)
        assert err != plain_err or h == 3
        err_l, _ = e.validation_error(hr, linear_loss=True, members=0x0F)
        _, out_l = e.validation_nodes(h, w)
        assert err_l == pytest.approx(err_of(out_l, hr, 3, True)[0], rel=1e-12)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_pair_validation_scores_the_ensemble_output(engines, precision):
    import rusty_sr_amd as r
    e = engines(precision)
    for i, (lh, lw, ch) in enumerate([(32, 32, 3), (21, 40, 4), (1, 1, 3)]):
        lr, hr = image_u8(600 + i, lh, lw, ch), image_u8(700 + i, 3 * lh, 3 * lw, 7 - ch)
        plain_err, plain_n = e.validation_error_pair(lr, hr)
        err, n = e.validation_error_pair(lr, hr, members=0xFF)
        assert n == plain_n == 27 * lh * lw
        node, out = e.validation_nodes(3 * lh, 3 * lw)
        np.testing.assert_array_equal(node, oracle.img_to_data(lr))
        np.testing.assert_array_equal(out, ensemble(lambda t: e.upscale_f32(t), node, 0xFF))
        assert err == pytest.approx(err_of(out, hr, 3, False)[0], rel=1e-12)
        assert err != plain_err or lh == 1
        assert r.validation_psnr([e], [hr], lr_images=[lr], members=0xFF) == -10 * math.log10(err / n)
    hr = image_u8(800, 60, 60)
    err, n = e.validation_error(hr, members=0x03)
    assert r.validation_psnr(e, [hr], members=0x03) == -10 * math.log10(err / n)
    assert r.validation_psnr(e, [hr]) != r.validation_psnr(e, [hr], members=0x03)


# ---- 5. it pays where the oracle says it pays --------------------------------------------------------------------------------
def psnr_of(out, hr):
    d = out.astype(np.float64) - crop(hr, 3).astype(np.float64)
    return -10 * math.log10(float(np.mean(d * d))), math.sqrt(float(np.mean(d * d)))


@pytest.mark.parametrize("key,name", [("imagenet", "butterfly_lr.png"), ("anime", "cartoon_lr.png")])
def test_ensemble_gains_what_the_oracle_gains(engines, params, key, name):
    hr = np.ascontiguousarray(load_png(name)[..., :3])
    lr64 = pool64(hr, 3)
    o_plain, rmse_plain = psnr_of(oracle.forward(params[key], lr64, f64=True)[0], hr)
    o_ens, rmse_ens = psnr_of(oracle_ensemble64(params[key], lr64), hr)
    e = engines("f32", key)
    err, n = e.validation_error(hr)
    g_plain = -10 * math.log10(err / n)
    err, n = e.validation_error(hr, members=0xFF)
    g_ens = -10 * math.log10(err / n)
    # an output within 1e-4 of the oracle's everywhere has an rmse within 1e-4 of the oracle's: 20 log10(1 + 1e-4 / rmse) dB
    b_plain, b_ens = 20 * math.log10(1 + TOL / rmse_plain), 20 * math.log10(1 + TOL / rmse_ens)
    print(f"[ensemble psnr] {key}/{name}: oracle {o_plain:.4f} -> {o_ens:.4f} dB, gpu {g_plain:.4f} -> {g_ens:.4f} dB, "
          f"bounds {b_plain:.4f} / {b_ens:.4f} dB")
    assert abs(g_plain - o_plain) <= b_plain
    assert abs(g_ens - o_ens) <= b_ens
    assert o_ens - o_plain > 2 * max(b_plain, b_ens), "the oracle's gain on this image no longer clears the bound: pick the cases again"
    assert g_ens > g_plain


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(engines, params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e = engines("f32")
    x = oracle.img_to_data(image_u8(1, 8, 9))
    px = image_u8(2, 8, 9, 4)

    def refused(fn, status=_lib.SR_E_INVALID):
        with pytest.raises(r.SrError) as err:
            fn()
        assert err.value.status == status

    for m in (0, 256, -1, 1 << 40):
        refused(lambda: e.upscale_ensemble_f32(x, members=m))
        refused(lambda: e.upscale_ensemble_rgba8(px, members=m))
        refused(lambda: e.validation_error(image_u8(3, 12, 12), members=m))
        refused(lambda: e.validation_error_pair(image_u8(3, 4, 4), image_u8(4, 12, 12), members=m))
    L = e._L
    tx, tpx = torch.from_numpy(x[None]).cuda(), torch.from_numpy(px[None]).cuda()
    stream = e._stream_ptr(None, tx.device)
    out = torch.full((24 * 27 * 3 + 1,), 7.0, dtype=torch.float32, device="cuda")
    out8 = torch.full((24 * 27 * 4 + 4,), 7, dtype=torch.uint8, device="cuda")
    for m in (0, 256):
        assert L.sr_upscale_ensemble_f32_dev(e._ctx, C.c_void_p(tx.data_ptr()), 1, 8, 9, C.c_void_p(out.data_ptr()), m, stream) == _lib.SR_E_INVALID
        assert L.sr_upscale_ensemble_rgba8_dev(e._ctx, C.c_void_p(tpx.data_ptr()), 4, 1, 8, 9, C.c_void_p(out8.data_ptr()), m, stream) == _lib.SR_E_INVALID
    # a misaligned output (and, f32, input) pointer
    assert L.sr_upscale_ensemble_f32_dev(e._ctx, C.c_void_p(tx.data_ptr()), 1, 8, 9, C.c_void_p(out.data_ptr() + 2), 0xFF, stream) == _lib.SR_E_INVALID
    assert L.sr_upscale_ensemble_f32_dev(e._ctx, C.c_void_p(tx.data_ptr() + 1), 1, 7, 9, C.c_void_p(out.data_ptr()), 0xFF, stream) == _lib.SR_E_INVALID
    assert L.sr_upscale_ensemble_rgba8_dev(e._ctx, C.c_void_p(tpx.data_ptr()), 4, 1, 8, 9, C.c_void_p(out8.data_ptr() + 1), 0xFF, stream) == _lib.SR_E_INVALID
    # the parameter-free graphs have no network to average
    for other in (r.bilinear_net(), r.downsample_net()):
        assert L.sr_upscale_ensemble_f32_dev(other._ctx, C.c_void_p(tx.data_ptr()), 1, 8, 9, C.c_void_p(out.data_ptr()), 0xFF, stream) == _lib.SR_E_INVALID
        assert L.sr_upscale_ensemble_rgba8_dev(other._ctx, C.c_void_p(tpx.data_ptr()), 4, 1, 8, 9, C.c_void_p(out8.data_ptr()), 0xFF, stream) == _lib.SR_E_INVALID
        refused(lambda: other.upscale_ensemble_f32(x))
        refused(lambda: other.upscale_ensemble_rgba8(px))
        other.close()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (out8 == 7).all()
    # A shape no device can hold is refused by the size check, before anything is allocated or launched (the buffers passed are tiny and
    # never touched); the context then still serves a plain call and an ensemble.
    for m in (0xFF, 0x03):
        assert L.sr_upscale_ensemble_f32_dev(e._ctx, C.c_void_p(tx.data_ptr()), 1, 400000, 400000, C.c_void_p(out.data_ptr()), m, stream) == _lib.SR_E_NOMEM
        assert L.sr_upscale_ensemble_rgba8_dev(e._ctx, C.c_void_p(tpx.data_ptr()), 4, 1, 400000, 400000, C.c_void_p(out8.data_ptr()), m, stream) == _lib.SR_E_NOMEM
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (out8 == 7).all()
    fresh = r.Engine(params["imagenet"])
    np.testing.assert_array_equal(e.upscale_f32(x), fresh.upscale_f32(x))
    np.testing.assert_array_equal(e.upscale_ensemble_rgba8(px), fresh.upscale_ensemble_rgba8(px))
    fresh.close()


# ---- 7. no leakage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_state_leaks_between_calls(params, precision):
    import rusty_sr_amd as r
    big, small = image_u8(900, 90, 131), image_u8(901, 37, 20, 4)
    xb, xs = oracle.img_to_data(big), oracle.img_to_data(small)

    def fresh(fn):
        e = r.Engine(params["imagenet"], precision=precision)
        try:
            return fn(e)
        finally:
            e.close()

    want_plain32, want_plain8 = fresh(lambda e: e.upscale_f32(xs)), fresh(lambda e: e.upscale_rgba8(small))
    want_small32, want_small8 = fresh(lambda e: e.upscale_ensemble_f32(xs)), fresh(lambda e: e.upscale_ensemble_rgba8(small, members=0xA5))
    e = r.Engine(params["imagenet"], precision=precision)
    try:
        e.upscale_ensemble_f32(xb)
        e.upscale_ensemble_rgba8(big)
        np.testing.assert_array_equal(e.upscale_f32(xs), want_plain32)
        np.testing.assert_array_equal(e.upscale_rgba8(small), want_plain8)
        e.upscale_ensemble_rgba8(big)
        np.testing.assert_array_equal(e.upscale_ensemble_f32(xs), want_small32)
        np.testing.assert_array_equal(e.upscale_ensemble_rgba8(small, members=0xA5), want_small8)
        np.testing.assert_array_equal(e.upscale_ensemble_f32(xs), want_small32)  # and the same bits on every run
    finally:
        e.close()
