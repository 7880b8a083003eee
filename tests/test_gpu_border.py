"""The border modes on the GPU (include/srhip.h "Borders"): the pad and the crop against their numpy restatement (tests/border_ref.py)
byte for byte, the composed calls bit for bit against the plain / ensemble call of the numpy-padded image cropped in numpy, seamlessness
itself, the oracle, the transparency composition, the refusals and the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_ref
import border_ref
import oracle
from conftest import ROOT, load_png, synth_u8
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
MODES = border_ref.MODES
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")
# 1 x 1, one row, both sides below the pad, whole groups, ragged rows, a wide row.  (No case here has two workgroups across: the widest,
# (64, 257) at pad 32, is 321 dwords a row in RGBA8 and 963 in f32, and a workgroup covers 1024.  Two workgroups across, in a batch and at
# every offset: tests/test_gpu_operator_grids.py.)
SHAPES = ((1, 1), (1, 37), (5, 3), (16, 16), (33, 61), (64, 257))
PADS = (0, 1, 7, 8, 32)
ALL8 = 0xFF   # the mask of all 8 members


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(precision="f32", key="imagenet", factor=3, graph="sr_net"):
        k = (precision, key, factor, graph)
        if k not in made:
            if graph != "sr_net":
                made[k] = r.Engine(graph=graph)
            else:
                p = params[key] if factor == 3 else synthetic_params(factor, 100 + factor)
                made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def offset_view(shape, dtype, offset):
    """A contiguous tensor of `shape` whose first byte lies `offset` bytes into a larger, 16-byte aligned allocation filled with 0xA5;
    and the whole allocation, as bytes."""
    import torch
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    whole = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    view = whole[offset:offset + nbytes]
    if np.dtype(dtype) == np.float32:
        view = view.view(torch.float32)
    view = view.view(*shape)
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view, whole


def guards_intact(whole, offset, nbytes):
    return bool((whole[:offset] == 0xA5).all() and (whole[offset + nbytes:] == 0xA5).all())


def random_image(rng, n, h, w, dtype):
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    bits = rng.integers(0, 1 << 32, (n, h, w, 3), dtype=np.uint64).astype(np.uint32)   # any bit pattern, NaNs included: the kernels only move dwords
    return bits.view(np.float32)


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def smooth_rgba(seed, n, h, w):
    px = np.empty((n, h, w, 4), np.uint8)
    px[..., :3], px[..., 3] = synth_u8(seed, n, h, w), 255
    return px


# ---- 1. the two launches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_pad_and_crop_are_the_restatement(engines, dtype, n):
    """Every shape, pad and mode; input at byte offset 4 and output at byte offset 12 of a larger allocation, so that the 16-byte groups
    and the ragged ends both run and source and destination disagree about where the groups lie; the bytes around the output stay."""
    import torch
    e = engines()
    rng = np.random.default_rng(n * 10 + np.dtype(dtype).itemsize)
    ch = 4 if np.dtype(dtype) == np.uint8 else 3
    item = np.dtype(dtype).itemsize
    for h, w in SHAPES:
        img = random_image(rng, n, h, w, dtype)
        src, _ = offset_view(img.shape, dtype, 4)
        src.copy_(torch.from_numpy(img))
        for p in PADS:
            H, W = h + 2 * p, w + 2 * p
            for mode in MODES:
                want = border_ref.pad(img, mode, p)
                dst, whole = offset_view((n, H, W, ch), dtype, 12)
                assert e.pad(src, mode, p, out=dst) is dst
                torch.cuda.synchronize()
                assert same_bytes(dst.cpu().numpy(), want), (h, w, p, mode)
                assert guards_intact(whole, 12, want.size * item), (h, w, p, mode)
                # the crop of it: the original back, and a window that starts and ends off every boundary
                for (y0, x0, wh, ww) in {(p, p, h, w), (H // 3, W // 3, H - H // 3 - (H > 2), W - W // 3 - (W > 2))}:
                    big, _ = offset_view(want.shape, dtype, 4)
                    big.copy_(torch.from_numpy(want))
                    out, whole = offset_view((n, wh, ww, ch), dtype, 12)
                    assert e.crop(big, y0, x0, wh, ww, out=out) is out
                    torch.cuda.synchronize()
                    assert same_bytes(out.cpu().numpy(), border_ref.crop(want, y0, x0, wh, ww)), (h, w, p, mode, y0, x0, wh, ww)
                    assert guards_intact(whole, 12, n * wh * ww * ch * item)
    # without out= the result is allocated, and the aligned-everywhere case runs too
    img = random_image(rng, n, 33, 64, dtype)
    got = e.pad(torch.from_numpy(img).cuda(), "mirror")
    assert same_bytes(got.cpu().numpy(), border_ref.pad(img, "mirror", 8))
    assert same_bytes(e.crop(got, 8, 8, 33, 64).cpu().numpy(), img)


# ---- 2. the composed calls ---------------------------------------------------------------------------------------------------
def plain_f32(e, x, members):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = e.upscale_f32_dev(t) if members == 1 else e.upscale_ensemble_f32_dev(t, members=members)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def plain_u8(e, px, members):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(px)).cuda()
    out = e.upscale_rgba8_dev(t) if members == 1 else e.upscale_ensemble_rgba8_dev(t, members=members)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("members", [1, ALL8], ids=["plain", "ensemble8"])
@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_composed_calls_are_the_plain_call_of_the_padded_image_cropped(engines, precision, factor, members):
    import torch
    e = engines(precision, factor=factor)
    for k, (h, w) in enumerate([(24, 40), (67, 45)]):
        mode, p = MODES[(k + factor + (members != 1)) % 3], (8, 7)[k]
        px = smooth_rgba(1000 * factor + h, 2, h, w)
        x = oracle.img_to_data(px[0])[None]
        # f32
        want = border_ref.centre(plain_f32(e, border_ref.pad(x, mode, p), members), factor, p)
        dev = e.upscale_f32_border_dev(torch.from_numpy(x).cuda(), mode, p, members)
        torch.cuda.synchronize()
        assert same_bytes(dev.cpu().numpy(), want), (h, w, mode, "f32 dev")
        assert same_bytes(e.upscale_f32_border(x, mode, p, members), want), (h, w, mode, "f32 host")
        # RGBA8, a batch of two
        want = border_ref.centre(plain_u8(e, border_ref.pad(px, mode, p), members), factor, p)
        assert (want[..., 3] == 255).all()
        dev = e.upscale_rgba8_border_dev(torch.from_numpy(px).cuda(), mode, p, members)
        torch.cuda.synchronize()
        assert same_bytes(dev.cpu().numpy(), want), (h, w, mode, "u8 dev")
        assert same_bytes(e.upscale_rgba8_border(px, mode, p, members), want), (h, w, mode, "u8 host")
        assert same_bytes(e.upscale_rgba8_border(px[0], mode, p, members), want[0])


@pytest.mark.parametrize("members", [0x03, 0x05])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_batch_with_an_ensemble_is_its_images(engines, precision, members):
    """A batch under a mask other than 1 runs the ensemble image by image, each from its own place in the padded buffer: byte for byte the
    single-image calls (which the test above holds to the primitives).  9 x 7: mask 0x05 runs a transposed member on a shape that is not
    square."""
    import torch
    e = engines(precision)
    rng = np.random.default_rng(members)
    px = rng.integers(0, 256, (2, 9, 7, 4), dtype=np.uint8)
    x = rng.random((2, 9, 7, 3), dtype=np.float32)
    got8, got32 = e.upscale_rgba8_border(px, "wrap", 8, members), e.upscale_f32_border(x, "wrap", 8, members)
    dev8 = e.upscale_rgba8_border_dev(torch.from_numpy(px).cuda(), "wrap", 8, members)
    dev32 = e.upscale_f32_border_dev(torch.from_numpy(x).cuda(), "wrap", 8, members)
    torch.cuda.synchronize()
    assert got8.shape == (2, 27, 21, 4) and got32.shape == (2, 27, 21, 3)
    assert not same_bytes(got8[0], got8[1]) and not same_bytes(got32[0], got32[1])
    for i in range(2):
        assert same_bytes(got8[i], e.upscale_rgba8_border(px[i], "wrap", 8, members)), (i, "u8 host")
        assert same_bytes(got32[i], e.upscale_f32_border(x[i], "wrap", 8, members)), (i, "f32 host")
        one8 = e.upscale_rgba8_border_dev(torch.from_numpy(px[i:i + 1]).cuda(), "wrap", 8, members)
        one32 = e.upscale_f32_border_dev(torch.from_numpy(x[i:i + 1]).cuda(), "wrap", 8, members)
        torch.cuda.synchronize()
        assert same_bytes(dev8[i].cpu().numpy(), one8[0].cpu().numpy()), (i, "u8 dev")
        assert same_bytes(dev32[i].cpu().numpy(), one32[0].cpu().numpy()), (i, "f32 dev")


def test_composed_call_where_the_plain_path_forks(engines):
    """A padded shape at sr_plan_fork's automatic threshold (exact f32, one image, fork_min_rounds = 3.5 rounds of 8-row tiles per
    resident workgroup, sr_plan.h sr_rounds): the padded image runs as two bands on two streams inside the composed call."""
    import torch
    e = engines("f32")
    p, W = 8, 900
    cus = e.device_info()["compute_units"]
    tiles_x = (W + 31) // 32
    H = 8 * -(-7 * cus // tiles_x)          # the fewest rows of 8-row tiles with rounds = tiles / (2 cus) >= 3.5
    assert tiles_x * (H // 8) / (2 * cus) >= 3.5 > tiles_x * (H // 8 - 1) / (2 * cus)
    h, w = H - 2 * p, W - 2 * p
    px = smooth_rgba(77, 1, h, w)
    x = oracle.img_to_data(px[0])[None]
    e.set_experiment("forktune", "0")   # the rule's decision, not the tuner's measurement
    try:
        e.set_experiment("fork", "0")
        want32 = border_ref.centre(plain_f32(e, border_ref.pad(x, "wrap", p), 1), 3, p)
        want8 = border_ref.centre(plain_u8(e, border_ref.pad(px, "wrap", p), 1), 3, p)
        assert e.last_plan()["fork"] == [(False, 0, 0)]
        e.set_experiment("fork", "")
        got32 = e.upscale_f32_border_dev(torch.from_numpy(x).cuda(), "wrap", p)
        fork32 = e.last_plan()["fork"]
        got8 = e.upscale_rgba8_border_dev(torch.from_numpy(px).cuda(), "wrap", p)
        fork8 = e.last_plan()["fork"]
        torch.cuda.synchronize()
        for rec in (fork32, fork8):
            assert len(rec) == 1 and rec[0][0] and rec[0][1] + rec[0][2] == H, rec
        assert same_bytes(got32.cpu().numpy(), want32) and same_bytes(got8.cpu().numpy(), want8)
    finally:
        e.set_experiment("fork", "")
        e.set_experiment("forktune", "1")


def test_composed_call_on_the_bilinear_graph(engines):
    e = engines(graph="bilinear")
    px = smooth_rgba(5, 1, 37, 53)
    for mode in MODES:
        want = border_ref.centre(plain_u8(e, border_ref.pad(px, mode, 8), 1), 3, 8)
        assert same_bytes(e.upscale_rgba8_border(px, mode), want)


# ---- 3. what it is for -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_wrap_is_the_centre_tile_of_the_tiled_image(engines, precision):
    """The wrap call on a 20 x 28 image against the centre tile of the plain call on its 3 x 3 tiling: the project's parity bar in f32
    (<= 1e-4; the tile plan may pair columns differently at another offset, so not a bit test); in RGBA8 at most one level, on fewer
    than 1e-3 of the values (what test_cli_end_to_end allows its goldens).  So a 2 x 2 tiling of the result has no seam: its inner
    edges are the inner edges of the tiled plane's upscale."""
    e = engines(precision)
    h, w, f = 20, 28, 3
    px = smooth_rgba(2028, 1, h, w)
    x = oracle.img_to_data(px[0])[None]
    tiled = plain_f32(e, np.tile(x, (1, 3, 3, 1)), 1)[0, f * h:2 * f * h, f * w:2 * f * w]
    got = e.upscale_f32_border(x, "wrap")[0]
    err = np.abs(got - tiled).max()
    print(f"wrap vs centre tile, {precision}: max |diff| = {err:.3g}")
    assert err <= 1e-4
    tiled8 = plain_u8(e, np.tile(px, (1, 3, 3, 1)), 1)[0, f * h:2 * f * h, f * w:2 * f * w]
    d = e.upscale_rgba8_border(px, "wrap")[0].astype(int) - tiled8.astype(int)
    print(f"wrap vs centre tile, {precision}, RGBA8: max level diff = {np.abs(d).max()}, share = {(d != 0).mean():.3g}")
    assert np.abs(d).max() <= 1 and (d != 0).mean() < 1e-3
    # ... and the plain call does have the seam: its border differs from the tiled plane's
    assert np.abs(plain_f32(e, x, 1)[0] - tiled).max() > 1e-2


@pytest.mark.parametrize("mode", MODES)
def test_f32_call_against_the_oracle(engines, params, mode):
    e = engines("f32")
    h, w, p = 23, 29, 8
    x = oracle.img_to_data(smooth_rgba(11, 1, h, w)[0])
    want = border_ref.centre(oracle.forward(params["imagenet"], border_ref.pad(x, mode, p))[0], 3, p)
    got = e.upscale_f32_border(x, mode, p)
    err = np.abs(got - want).max()
    print(f"{mode} vs oracle: max |diff| = {err:.3g}")
    assert got.shape == want.shape and err <= 1e-4


# ---- 4. with transparency ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bleed_on_an_opaque_image_gives_the_opaque_call(engines, precision):
    e = engines(precision)
    px = smooth_rgba(21, 1, 40, 70)
    for members in (1, 0x0F):
        want = e.upscale_rgba8_border(px, "wrap", members=members)
        for bleed in (0, 8, 16):
            assert same_bytes(e.upscale_rgba8_border(px, "wrap", members=members, bleed=bleed), want), (members, bleed)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bleed_on_a_sprite_is_the_composition_step_by_step(engines, precision):
    """Byte 3 is sr_upscale_rgba8_alpha's; RGB is bleed -> pad -> plain call -> crop done with Engine.bleed, Engine.pad, the plain device
    call and Engine.crop; the merge with Engine.merge_alpha gives the whole result."""
    import torch
    e = engines(precision)
    h, w, f, p = 37, 129, 3, 8
    px = alpha_ref.alpha_pattern("dense", h, w, 8, 5)
    visible = px[..., 3] > 0
    px[visible, :3] = synth_u8(5, 1, h, w)[0][visible]
    assert 0 < visible.mean() < 1
    t = torch.from_numpy(px[None]).cuda()
    for mode, bleed in (("wrap", 8), ("mirror", 0), ("replicate", 3)):
        got = e.upscale_rgba8_border(px, mode, p, bleed=bleed)
        np.testing.assert_array_equal(got[..., 3], e.upscale_rgba8_alpha(px, bleed=bleed)[..., 3])
        np.testing.assert_array_equal(got[..., 3], alpha_ref.up_alpha(px[..., 3], f))
        big = e.upscale_rgba8_dev(e.pad(e.bleed(t, bleed), mode, p))
        steps = e.crop(big, f * p, f * p, f * h, f * w)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got[..., :3], steps.cpu().numpy()[0, ..., :3])
        merged = e.merge_alpha(t, steps)
        torch.cuda.synchronize()
        assert same_bytes(merged.cpu().numpy()[0], got)
        dev = e.upscale_rgba8_border_dev(t, mode, p, bleed=bleed)
        torch.cuda.synchronize()
        assert same_bytes(dev.cpu().numpy()[0], got)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(engines, params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil = engines(), engines(graph="bilinear")
    h, w, f = 8, 9, 3
    px = smooth_rgba(1, 1, h, w)
    x = oracle.img_to_data(px[0])[None]
    plain_before = e.upscale_rgba8(px)
    tpx, tx = torch.from_numpy(px).cuda(), torch.from_numpy(x).cuda()
    out, whole = offset_view((f * h * f * w * 12 + 4096,), np.uint8, 0)   # room for every output asked for below
    L, INV = e._L, _lib.SR_E_INVALID
    stream = e._stream_ptr(None, tpx.device)
    p8, p32, p_out = C.c_void_p(tpx.data_ptr()), C.c_void_p(tx.data_ptr()), C.c_void_p(out.data_ptr())
    down = r.downsample_net()

    def u8(ctx=e._ctx, src=p8, n=1, hh=h, ww=w, dst=p_out, mode=1, pad=8, members=1, bleed=-1):
        return L.sr_upscale_rgba8_border_dev(ctx, src, n, hh, ww, dst, mode, pad, members, bleed, stream)

    def f32(ctx=e._ctx, src=p32, n=1, hh=h, ww=w, dst=p_out, mode=1, pad=8, members=1):
        return L.sr_upscale_f32_border_dev(ctx, src, n, hh, ww, dst, mode, pad, members, stream)

    for mode in (0, 4, -1, 1 << 20):
        assert u8(mode=mode) == INV and f32(mode=mode) == INV
        assert L.sr_pad_rgba8_dev(e._ctx, p8, 1, h, w, mode, 8, p_out, stream) == INV
        assert L.sr_pad_f32_dev(e._ctx, p32, 1, h, w, mode, 8, p_out, stream) == INV
    for pad in (-1, 0, 6, 33, 1 << 20):   # below SR_HALO or above SR_BORDER_PAD_MAX
        assert u8(pad=pad) == INV and f32(pad=pad) == INV
    for pad in (-1, 33, 1 << 20):         # the primitives take 0 .. SR_BORDER_PAD_MAX
        assert L.sr_pad_rgba8_dev(e._ctx, p8, 1, h, w, 1, pad, p_out, stream) == INV
        assert L.sr_pad_f32_dev(e._ctx, p32, 1, h, w, 1, pad, p_out, stream) == INV
    assert u8(ctx=down._ctx) == INV and f32(ctx=down._ctx) == INV                  # graphs other than sr_net / bilinear
    for members in (0, 256, 1 << 20):
        assert u8(members=members) == INV and f32(members=members) == INV
    for members in (0, 3, 0xFF, 256):                                             # members != 1 on the bilinear graph
        assert u8(ctx=bil._ctx, members=members) == INV and f32(ctx=bil._ctx, members=members) == INV
    for bleed in (-2, 17, 1 << 20):
        assert u8(bleed=bleed) == INV
    for off in (1, 2, 3):                                                         # misaligned pointers
        bad_out, bad8, bad32 = C.c_void_p(out.data_ptr() + off), C.c_void_p(tpx.data_ptr() + off), C.c_void_p(tx.data_ptr() + off)
        assert u8(dst=bad_out) == INV and u8(src=bad8) == INV and f32(dst=bad_out) == INV and f32(src=bad32) == INV
        assert L.sr_pad_rgba8_dev(e._ctx, p8, 1, h, w, 1, 8, bad_out, stream) == INV
        assert L.sr_pad_f32_dev(e._ctx, bad32, 1, h, w, 1, 8, p_out, stream) == INV
        assert L.sr_crop_rgba8_dev(e._ctx, p8, 1, h, w, 0, 0, h, w, bad_out, stream) == INV
        assert L.sr_crop_f32_dev(e._ctx, bad32, 1, h, w, 0, 0, h, w, p_out, stream) == INV
    for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w)):
        assert u8(n=n, hh=hh, ww=ww) == INV and f32(n=n, hh=hh, ww=ww) == INV
        assert L.sr_pad_rgba8_dev(e._ctx, p8, n, hh, ww, 1, 8, p_out, stream) == INV
    assert u8(src=None) == INV and u8(dst=None) == INV and L.sr_pad_rgba8_dev(e._ctx, p8, 1, h, w, 1, 8, p8, stream) == INV
    # a crop window that is not inside its image
    for (y0, x0, ch, cw) in ((-1, 0, h, w), (0, -1, h, w), (1, 0, h, w), (0, 1, h, w), (0, 0, h + 1, w), (0, 0, h, 0), (0, 0, 0, w),
                             (h, 0, 1, 1), (0, w, 1, 1), (2 ** 31 - 1, 0, 1, 1), (0, 0, 2 ** 31 - 1, w)):
        assert L.sr_crop_rgba8_dev(e._ctx, p8, 1, h, w, y0, x0, ch, cw, p_out, stream) == INV, (y0, x0, ch, cw)
        assert L.sr_crop_f32_dev(e._ctx, p32, 1, h, w, y0, x0, ch, cw, p_out, stream) == INV, (y0, x0, ch, cw)
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    # the host forms, through the binding
    host_out = np.full((f * h, f * w, 4), 0xA5, np.uint8)
    for call in (lambda: e.upscale_rgba8_border(px, 0, out=host_out), lambda: e.upscale_rgba8_border(px, "wrap", 6, out=host_out),
                 lambda: e.upscale_rgba8_border(px, "wrap", 33, out=host_out), lambda: e.upscale_rgba8_border(px, members=0, out=host_out),
                 lambda: e.upscale_rgba8_border(px, bleed=17, out=host_out), lambda: bil.upscale_rgba8_border(px, members=3, out=host_out),
                 lambda: down.upscale_rgba8_border(px), lambda: e.upscale_f32_border(x, 4), lambda: e.upscale_f32_border(x, "mirror", 6),
                 lambda: bil.upscale_f32_border(x, members=ALL8), lambda: e.pad(tpx, "wrap", 33), lambda: e.crop(tpx, 1, 0, h, w)):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    with pytest.raises(ValueError):
        e.upscale_rgba8_border(px, "zero")
    assert (host_out == 0xA5).all()
    down.close()
    # shapes whose padded size no device can hold, or that overflow, are SR_E_NOMEM by arithmetic, before anything is launched
    assert u8(hh=400000, ww=400000) == _lib.SR_E_NOMEM and f32(hh=400000, ww=400000) == _lib.SR_E_NOMEM
    edge = (2 ** 31 - 1) // f
    assert u8(hh=edge, ww=edge) == _lib.SR_E_NOMEM and f32(hh=edge, ww=4) == _lib.SR_E_NOMEM and u8(hh=4, ww=edge - 15, bleed=8) == _lib.SR_E_NOMEM
    assert u8(n=2 ** 31 - 1, hh=60000, ww=60000) == _lib.SR_E_NOMEM
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    # ... and the context still serves: the plain call is bit for bit what it was, the border call what a fresh context computes
    assert same_bytes(e.upscale_rgba8(px), plain_before)
    fresh = r.Engine(params["imagenet"])
    assert same_bytes(e.upscale_rgba8_border(px, "wrap"), fresh.upscale_rgba8_border(px, "wrap"))
    fresh.close()


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_border(engines, tmp_path):
    from PIL import Image
    from rusty_sr_amd.build import build_host
    build_host()
    e = engines()
    gh, gw = load_png("logo_rs.png").shape[:2]
    h, w = gh // 3, gw // 3   # the size of the logo golden's LR image
    px = smooth_rgba(31, 1, h, w)[0]
    src, out = tmp_path / "in.png", tmp_path / "out.png"
    Image.fromarray(px).save(src)

    def run(*args, source=src, text="Upscaling using imagenet neural net parameters... Writing file... Done\n"):
        res = subprocess.run([CLI, str(source), str(out), *args], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert res.stdout == text
        if "--timing" in args:  # the border call times itself: every launch between the two copies
            kernels, h2d, d2h = map(float, re.search(r"kernels ([\d.]+) ms, h2d ([\d.]+) ms, d2h ([\d.]+) ms", res.stderr).groups())
            assert kernels > 0 and h2d > 0 and d2h > 0, res.stderr
        got = np.array(Image.open(out).convert("RGBA"))
        assert got.shape == (3 * h, 3 * w, 4)
        return got

    assert same_bytes(run("--border", "wrap"), e.upscale_rgba8_border(px, "wrap"))
    assert same_bytes(run("--border=mirror", "--border-pad", "7", "--timing"), e.upscale_rgba8_border(px, "mirror", 7))
    assert same_bytes(run("--border", "replicate", "--ensemble", "4", "--precision", "split_f16"),
                      engines("split_f16").upscale_rgba8_border(px, "replicate", members=0x0F))
    assert same_bytes(run("--border", "wrap", "-p", "bilinear", text="Upscaling using bilinear interpolation... Writing file... Done\n"),
                      engines(graph="bilinear").upscale_rgba8_border(px, "wrap"))
    plain = run()
    assert same_bytes(plain, e.upscale_rgba8(px)) and not same_bytes(plain, e.upscale_rgba8_border(px, "wrap"))
    # --alpha: a PNG with the sprite's alpha
    sprite = alpha_ref.alpha_pattern("dense", h, w, 8, 9)
    vis = sprite[..., 3] > 0
    sprite[vis, :3] = px[vis, :3]
    ssrc = tmp_path / "sprite.png"
    Image.fromarray(sprite).save(ssrc)
    got = run("--border", "wrap", "--alpha", source=ssrc)
    assert same_bytes(got, e.upscale_rgba8_border(sprite, "wrap", bleed=8))
    np.testing.assert_array_equal(got[..., 3], alpha_ref.up_alpha(sprite[..., 3], 3))
    assert same_bytes(run("--border", "wrap", "--alpha", "--bleed", "4", source=ssrc), e.upscale_rgba8_border(sprite, "wrap", bleed=4))
