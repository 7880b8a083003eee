"""The transparency path on the GPU (include/srhip.h "Transparency"): the bleed and the alpha merge against their numpy restatement
(tests/alpha_ref.py), the whole call against the plain / ensemble call of the bled image, all bit for bit; what the bleed is for; the
refusals; the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_ref
from conftest import ROOT, synth_u8
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
RADII = (0, 1, 7, 8, 16)
PATTERNS = ("sparse", "dense", "opaque", "transparent", "corner", "hole")
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


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


def rgba_image(seed, h, w, pattern="sparse", radius=8):
    """A smooth picture (the network's trained range) under one of the alpha patterns; arbitrary colours stay under alpha 0."""
    px = alpha_ref.alpha_pattern(pattern, h, w, radius, seed)
    visible = px[..., 3] > 0
    px[visible, :3] = synth_u8(seed, 1, h, w)[0][visible]
    return px


def offset_view(nbytes, offset):
    """nbytes of device memory `offset` bytes into a larger allocation filled with 0xA5, and the whole allocation."""
    import torch
    whole = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + nbytes], whole


# ---- 1. bleed ----------------------------------------------------------------------------------------------------------------
def test_bleed_tile_is_what_the_shapes_assume():
    from rusty_sr_amd import _lib
    assert _lib.SR_ALPHA_BLEED_TILE == 32  # (33, 65) below crosses the seams, (64, 64) ends on them


@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (5, 1), (7, 9), (33, 65), (64, 64)])
def test_bleed_is_the_restatement(engines, h, w):
    import torch
    e = engines()
    for i, pattern in enumerate(PATTERNS):
        for radius in RADII:
            px = alpha_ref.alpha_pattern(pattern, h, w, radius, seed=1000 * h + 10 * w + i)
            want = alpha_ref.bleed(px, radius)
            got = e.bleed(torch.from_numpy(px[None]).cuda(), radius)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got.cpu().numpy()[0], want, err_msg=f"{pattern}, R = {radius}")
            if pattern in ("opaque", "transparent") or radius == 0:
                np.testing.assert_array_equal(want, px)
            if pattern == "hole" and min(h, w) // 2 >= alpha_ref.hole_radius(radius):  # the whole disc is inside the image
                assert (want[h // 2, w // 2] == px[h // 2, w // 2]).all() and px[h // 2, w // 2, 3] == 0  # its middle is out of reach


def test_bleed_keeps_the_images_of_a_batch_apart(engines):
    import torch
    e = engines()
    h, w = 33, 65
    opaque, clear = alpha_ref.alpha_pattern("opaque", h, w, 8, 1), alpha_ref.alpha_pattern("transparent", h, w, 8, 2)
    mixed = alpha_ref.alpha_pattern("sparse", h, w, 8, 3)
    for batch in (np.stack([opaque, clear]), np.stack([clear, opaque]), np.stack([mixed, clear, opaque])):
        got = e.bleed(torch.from_numpy(batch).cuda(), 16).cpu().numpy()
        np.testing.assert_array_equal(got, alpha_ref.bleed(batch, 16))
    got = e.bleed(np.stack([opaque, clear]), 16)  # (numpy in, numpy out)
    np.testing.assert_array_equal(got, np.stack([opaque, clear]))


def test_bleed_at_a_four_byte_offset(engines):
    import torch
    e = engines()
    h, w = 33, 65
    px = alpha_ref.alpha_pattern("sparse", h, w, 8, 77)
    src, _ = offset_view(h * w * 4, 4)
    dst, whole = offset_view(h * w * 4, 12)
    assert src.data_ptr() % 16 == 4 and dst.data_ptr() % 16 == 12
    src.copy_(torch.from_numpy(px.reshape(-1)))
    e.bleed(src.view(1, h, w, 4), 8, out=dst.view(1, h, w, 4))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dst.cpu().numpy().reshape(h, w, 4), alpha_ref.bleed(px, 8))
    assert (whole[:12] == 0xA5).all() and (whole[12 + h * w * 4:] == 0xA5).all()


# ---- 2. merge ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 3, 4])
def test_merge_is_the_restatement_and_leaves_the_colours(engines, factor):
    import torch
    e = engines(factor=factor)
    for h, w in [(1, 1), (1, 5), (5, 1), (37, 129), (40, 70)]:
        rng = np.random.default_rng(factor * 100000 + h * 100 + w)
        lr = rng.integers(0, 256, (2, h, w, 4), dtype=np.uint8)
        hr = rng.integers(0, 256, (2, factor * h, factor * w, 4), dtype=np.uint8)
        out = torch.from_numpy(hr).cuda()
        assert e.merge_alpha(torch.from_numpy(lr).cuda(), out) is out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[..., :3], hr[..., :3], err_msg=f"colours, {h}x{w}")
        np.testing.assert_array_equal(got[..., 3], alpha_ref.up_alpha(lr[..., 3], factor), err_msg=f"alpha, {h}x{w}")
    # constant alpha stays constant
    lr = np.zeros((1, 9, 11, 4), np.uint8)
    for value in (0, 1, 200, 255):
        lr[..., 3] = value
        got = e.merge_alpha(lr, np.zeros((1, 9 * factor, 11 * factor, 4), np.uint8))
        assert (got[..., 3] == value).all() and (got[..., :3] == 0).all()


@pytest.mark.parametrize("factor,offset", [(2, 4), (3, 8), (3, 12), (4, 4)])
def test_merge_at_a_four_byte_offset(engines, factor, offset):
    import torch
    e = engines(factor=factor)
    h, w = 7, 9  # rows of 4 f w = 72 / 108 / 144 bytes: with 108 every row starts at another offset from a 16-byte boundary
    rng = np.random.default_rng(offset * 10 + factor)
    lr = rng.integers(0, 256, (1, h, w, 4), dtype=np.uint8)
    hr = rng.integers(0, 256, (1, factor * h, factor * w, 4), dtype=np.uint8)
    src, _ = offset_view(lr.size, 4)
    dst, whole = offset_view(hr.size, offset)
    src.copy_(torch.from_numpy(lr.reshape(-1)))
    dst.copy_(torch.from_numpy(hr.reshape(-1)))
    e.merge_alpha(src.view(lr.shape), dst.view(hr.shape))
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(hr.shape)
    np.testing.assert_array_equal(got[..., :3], hr[..., :3])
    np.testing.assert_array_equal(got[..., 3], alpha_ref.up_alpha(lr[..., 3], factor))
    assert (whole[:offset] == 0xA5).all() and (whole[offset + hr.size:] == 0xA5).all()


# ---- 3. the whole call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h,w", [(1, 1), (37, 129), (40, 70), (256, 256)])
def test_whole_call_is_the_plain_call_of_the_bled_image_under_the_upscaled_alpha(engines, precision, h, w):
    import torch
    e = engines(precision)
    px = rgba_image(h * 1000 + w, h, w, "dense" if h > 1 else "opaque")
    plain_before = e.upscale_rgba8(px)
    for radius in (8, 3, 0):
        want = e.upscale_rgba8(alpha_ref.bleed(px, radius))
        assert (want[..., 3] == 255).all()
        want[..., 3] = alpha_ref.up_alpha(px[..., 3], 3)
        got = e.upscale_rgba8_alpha(px, bleed=radius)
        np.testing.assert_array_equal(got, want, err_msg=f"R = {radius}")
        dev = e.upscale_rgba8_alpha_dev(torch.from_numpy(px[None]).cuda(), bleed=radius)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dev.cpu().numpy()[0], got, err_msg=f"dev, R = {radius}")
        np.testing.assert_array_equal(e.upscale_rgba8_alpha(px, bleed=radius), got, err_msg=f"second call, R = {radius}")
    np.testing.assert_array_equal(e.upscale_rgba8(px), plain_before)  # the plain call is what it was


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("members", [0xFF, 0x03])
def test_whole_call_with_an_ensemble(engines, precision, members):
    import torch
    e = engines(precision)
    px = rgba_image(members, 37, 129, "sparse")
    want = e.upscale_ensemble_rgba8(alpha_ref.bleed(px, 8), members=members)
    want[..., 3] = alpha_ref.up_alpha(px[..., 3], 3)
    got = e.upscale_rgba8_alpha(px, members=members)
    np.testing.assert_array_equal(got, want)
    dev = e.upscale_rgba8_alpha_dev(torch.from_numpy(px[None]).cuda(), members=members)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy()[0], got)


@pytest.mark.parametrize("factor", [2, 4])
def test_whole_call_at_other_factors(engines, factor):
    e = engines(factor=factor)
    px = rgba_image(factor, 40, 70, "dense")
    want = e.upscale_rgba8(alpha_ref.bleed(px, 8))
    want[..., 3] = alpha_ref.up_alpha(px[..., 3], factor)
    got = e.upscale_rgba8_alpha(px)
    assert got.shape == (40 * factor, 70 * factor, 4)
    np.testing.assert_array_equal(got, want)


def test_whole_call_on_the_bilinear_graph(engines):
    import torch
    e = engines(graph="bilinear")
    px = rgba_image(5, 37, 129, "dense")
    want = e.upscale_rgba8(alpha_ref.bleed(px, 8))
    want[..., 3] = alpha_ref.up_alpha(px[..., 3], 3)
    np.testing.assert_array_equal(e.upscale_rgba8_alpha(px), want)
    dev = e.upscale_rgba8_alpha_dev(torch.from_numpy(px[None]).cuda())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy()[0], want)


def test_whole_call_on_a_batch(engines):
    e = engines()
    batch = np.stack([rgba_image(11, 19, 45, "sparse"), rgba_image(12, 19, 45, "transparent")])
    got = e.upscale_rgba8_alpha(batch)
    assert got.shape == (2, 57, 135, 4)
    for i in range(2):
        np.testing.assert_array_equal(got[i], e.upscale_rgba8_alpha(batch[i]))
    want = e.upscale_rgba8(alpha_ref.bleed(batch, 8))
    want[..., 3] = alpha_ref.up_alpha(batch[..., 3], 3)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("members", [0x03, 0x05])
def test_a_batch_with_an_ensemble_is_its_images(engines, precision, members):
    """A batch under a mask other than 1 runs the ensemble image by image: byte for byte the single-image calls (which the tests above
    hold to the primitives).  9 x 7: mask 0x05 runs a transposed member on a shape that is not square."""
    import torch
    e = engines(precision)
    batch = np.random.default_rng(members).integers(0, 256, (2, 9, 7, 4), dtype=np.uint8)
    got = e.upscale_rgba8_alpha(batch, bleed=8, members=members)
    dev = e.upscale_rgba8_alpha_dev(torch.from_numpy(batch).cuda(), bleed=8, members=members)
    torch.cuda.synchronize()
    assert got.shape == (2, 27, 21, 4)
    assert not np.array_equal(got[0], got[1])
    for i in range(2):
        np.testing.assert_array_equal(got[i], e.upscale_rgba8_alpha(batch[i], bleed=8, members=members), err_msg=f"image {i}")
        one = e.upscale_rgba8_alpha_dev(torch.from_numpy(batch[i:i + 1]).cuda(), bleed=8, members=members)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dev[i].cpu().numpy(), one[0].cpu().numpy(), err_msg=f"image {i}, device call")
    np.testing.assert_array_equal(dev.cpu().numpy(), got)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_opaque_image_gives_the_plain_call(engines, precision):
    e = engines(precision)
    px = rgba_image(21, 40, 70, "opaque")
    px[..., 3] = 255
    want = e.upscale_rgba8(px)
    for members in (1, 0x0F):
        if members != 1:
            want = e.upscale_ensemble_rgba8(px, members=members)
        np.testing.assert_array_equal(e.upscale_rgba8_alpha(px, members=members), want)


# ---- 4. the point of the bleed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_visible_pixels_of_a_constant_sprite_see_no_edge(engines, precision):
    """Every LR pixel within SR_HALO of a visible one is the sprite's colour after a bleed of 8, so the network's output under the visible
    pixels is what it makes of an image of that colour everywhere; without the bleed it sees the edge to black."""
    e = engines(precision, "anime")
    colour = (200, 120, 40)
    px, _ = alpha_ref.disc_sprite(colour)
    flat = np.empty_like(px)
    flat[..., :3], flat[..., 3] = colour, 255
    want = e.upscale_rgba8(flat)[..., :3]
    under_visible = np.repeat(np.repeat(px[..., 3] > 0, 3, axis=0), 3, axis=1)
    bled = e.upscale_rgba8_alpha(px, bleed=8)[..., :3]
    np.testing.assert_array_equal(bled[under_visible], want[under_visible])
    raw = e.upscale_rgba8_alpha(px, bleed=0)[..., :3]
    assert (raw[under_visible] != want[under_visible]).any()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(engines, params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil = engines(), engines(graph="bilinear")
    h, w = 8, 9
    px = rgba_image(1, h, w, "sparse")
    tpx = torch.from_numpy(px[None]).cuda()
    out, whole = offset_view(3 * h * 3 * w * 4, 16)
    same, whole_same = offset_view(h * w * 4, 16)
    L, INV = e._L, _lib.SR_E_INVALID
    stream = e._stream_ptr(None, tpx.device)
    p_in, p_out, p_same = C.c_void_p(tpx.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(same.data_ptr())
    down = r.downsample_net()
    assert L.sr_upscale_rgba8_alpha_dev(down._ctx, p_in, 1, h, w, p_out, 8, 1, stream) == INV
    assert L.sr_merge_alpha_rgba8_dev(down._ctx, p_in, 1, h, w, p_out, stream) == INV
    for radius in (-1, 17, 1 << 20):
        assert L.sr_upscale_rgba8_alpha_dev(e._ctx, p_in, 1, h, w, p_out, radius, 1, stream) == INV
        assert L.sr_bleed_rgba8_dev(e._ctx, p_in, 1, h, w, radius, p_same, stream) == INV
    for members in (0, 256, 1 << 20):
        assert L.sr_upscale_rgba8_alpha_dev(e._ctx, p_in, 1, h, w, p_out, 8, members, stream) == INV
    for members in (0, 3, 0xFF, 256):
        assert L.sr_upscale_rgba8_alpha_dev(bil._ctx, p_in, 1, h, w, p_out, 8, members, stream) == INV
    for off in (1, 2, 3):
        assert L.sr_upscale_rgba8_alpha_dev(e._ctx, p_in, 1, h, w, C.c_void_p(out.data_ptr() + off), 8, 1, stream) == INV
        assert L.sr_merge_alpha_rgba8_dev(e._ctx, p_in, 1, h, w, C.c_void_p(out.data_ptr() + off), stream) == INV
        assert L.sr_bleed_rgba8_dev(e._ctx, p_in, 1, h, w, 8, C.c_void_p(same.data_ptr() + off), stream) == INV
    assert L.sr_bleed_rgba8_dev(e._ctx, p_same, 1, h, w, 8, p_same, stream) == INV  # in place
    for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0)):
        assert L.sr_upscale_rgba8_alpha_dev(e._ctx, p_in, n, hh, ww, p_out, 8, 1, stream) == INV
    torch.cuda.synchronize()
    assert (whole == 0xA5).all() and (whole_same == 0xA5).all()
    # the host forms, through the binding
    host_out = np.full((3 * h, 3 * w, 4), 0xA5, np.uint8)
    for call in (lambda: e.upscale_rgba8_alpha(px, bleed=17, out=host_out), lambda: e.upscale_rgba8_alpha(px, bleed=-1, out=host_out),
                 lambda: e.upscale_rgba8_alpha(px, members=0, out=host_out), lambda: e.upscale_rgba8_alpha(px, members=256, out=host_out),
                 lambda: bil.upscale_rgba8_alpha(px, members=3, out=host_out), lambda: down.upscale_rgba8_alpha(px),
                 lambda: e.bleed(tpx, 17)):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    assert (host_out == 0xA5).all()
    down.close()
    # a shape no device can hold is SR_E_NOMEM before anything is launched, and the context still serves
    assert L.sr_upscale_rgba8_alpha_dev(e._ctx, p_in, 1, 400000, 400000, p_out, 8, 1, stream) == _lib.SR_E_NOMEM
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    fresh = r.Engine(params["imagenet"])
    np.testing.assert_array_equal(e.upscale_rgba8_alpha(px), fresh.upscale_rgba8_alpha(px))
    fresh.close()


# ---- 6. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_keeps_transparency(engines, tmp_path):
    from PIL import Image
    from rusty_sr_amd.build import build_host
    build_host()
    e = engines()
    px = rgba_image(31, 40, 70, "dense")
    src, out = tmp_path / "in.png", tmp_path / "out.png"
    Image.fromarray(px).save(src)

    def run(*args):
        res = subprocess.run([CLI, str(src), str(out), *args], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert res.stdout == "Upscaling using imagenet neural net parameters... Writing file... Done\n"
        if "--timing" in args:  # the alpha call times itself: bleed, network and merge between the two copies
            kernels, h2d, d2h = map(float, re.search(r"kernels ([\d.]+) ms, h2d ([\d.]+) ms, d2h ([\d.]+) ms", res.stderr).groups())
            assert kernels > 0 and h2d > 0 and d2h > 0, res.stderr
        got = np.array(Image.open(out))
        assert got.shape == (120, 210, 4)
        return got

    np.testing.assert_array_equal(run("--alpha"), e.upscale_rgba8_alpha(px))
    np.testing.assert_array_equal(run("--alpha", "--timing"), e.upscale_rgba8_alpha(px))
    np.testing.assert_array_equal(run("--alpha", "--ensemble", "4", "--bleed", "4"), e.upscale_rgba8_alpha(px, bleed=4, members=0x0F))
    plain = run()
    assert (plain[..., 3] == 255).all()
    np.testing.assert_array_equal(plain, e.upscale_rgba8(px))
