"""Resampling to any size on the GPU (include/srhip.h "Resampling to any size"): sr_resize_dev against the numpy restatement
(tests/resize_ref.py), against the two parameter-free graphs, the _sized calls as the composition they are documented to be, the refusals,
streams and offsets, and the CLI end to end."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref
from conftest import ROOT, load_png, synth_u8
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the bar tests/test_gpu_parity.py holds the parameter-free graphs to
FILTERS = resize_ref.FILTERS
# (h, w) -> (oh, ow): the identity, up- and downscales, 126 taps an axis, either side of a wave's 64 columns and of a 256-thread block
SHAPES = [((1, 1), (1, 1)), ((1, 1), (4, 5)), ((7, 9), (3, 4)), ((5, 31), (8, 50)), ((33, 17), (33, 17)), ((3, 2), (64, 48)),
          ((64, 48), (3, 2)), ((9, 257), (5, 129)), ((9, 255), (5, 127)), ((130, 70), (43, 23))]
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(factor=3, graph="sr_net"):
        k = (factor, graph)
        if k not in made:
            if graph != "sr_net":
                made[k] = r.Engine(graph=graph)
            else:
                made[k] = r.Engine(params["imagenet"] if factor == 3 else synthetic_params(factor, 100 + factor), device=0, factor=factor)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def rgba(seed, n, h, w):
    """Seeded RGBA bytes: noise, the left half dark (bytes below 16: the transfer function's linear branch), a random alpha plane."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    px[:, :, : w // 2, :3] //= 16
    return px


_refs = {}


def reference(seed, shape, size, name, srgb_space):
    """The restatement of image `seed` of that shape, computed once: from byte / 255 as f32, which is what both input kinds hold."""
    key = (seed, shape, size, name, srgb_space)
    if key not in _refs:
        x = (rgba(seed, 1, *shape)[..., :3].astype(np.float32) / np.float32(255.0)).astype(np.float64)
        _refs[key] = resize_ref.resize(x, size, name, srgb_space)
    return _refs[key]


def run(eng, px, size, name, srgb_space, in_kind, out_kind):
    import torch
    x = torch.from_numpy(px if in_kind == "rgba8" else px[..., :3].astype(np.float32) / np.float32(255.0)).cuda()
    return eng.resize_dev(x, size, out_kind, name, srgb_space).cpu().numpy()


def seed_of(shape, size):
    return shape[0] * 100003 + shape[1] * 1009 + size[0] * 31 + size[1]


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("srgb_space", [False, True])
@pytest.mark.parametrize("in_kind", ["rgba8", "f32"])
def test_f32_output_against_the_restatement(engines, name, srgb_space, in_kind):
    eng = engines(graph="bilinear")  # any context: no parameters are used
    worst = 0.0
    for shape, size in SHAPES:
        seed = seed_of(shape, size)
        got = run(eng, rgba(seed, 1, *shape), size, name, srgb_space, in_kind, "f32")
        want = reference(seed, shape, size, name, srgb_space)
        assert got.shape == want.shape == (1,) + size + (3,)
        err = float(np.abs(got - want).max())
        print(f"{name} srgb_space={srgb_space} {in_kind} {shape}->{size}: max abs {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL


# The horizontal pass stages the input under a workgroup's 256 columns in LDS, four rows at a time, one row where four do not fit, and
# reads from global memory where not even one does (sr_resize.hip): a width on every side of those thresholds, and more than one
# workgroup across a row in each staged form.
FORM_SHAPES = [((6, 900), (5, 600)), ((3, 100), (9, 300)), ((2, 1000), (2, 250)), ((5, 2100), (3, 520)), ((2, 3500), (3, 100))]


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("in_kind", ["rgba8", "f32"])
def test_every_form_of_the_horizontal_pass(engines, name, in_kind):
    eng = engines(graph="bilinear")
    worst = 0.0
    for shape, size in FORM_SHAPES:
        seed = seed_of(shape, size)
        got = run(eng, rgba(seed, 1, *shape), size, name, False, in_kind, "f32")
        want = reference(seed, shape, size, name, False)
        err = float(np.abs(got - want).max())
        print(f"{name} {in_kind} {shape}->{size}: max abs {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL


def test_rgba8_output_by_the_u8_rule(engines):
    """|d| <= 1, every differing byte within 255 x 1e-4 of a rounding knife-edge of the restatement, alpha 255; the differing share pooled
    over all cases (the inputs are seeded: one flipped byte of a 12-byte image must not decide it)."""
    eng = engines(graph="bilinear")
    differing = total = 0
    for name in FILTERS:
        for srgb_space in (False, True):
            for in_kind in ("rgba8", "f32"):
                for shape, size in SHAPES:
                    seed = seed_of(shape, size)
                    got = run(eng, rgba(seed, 1, *shape), size, name, srgb_space, in_kind, "rgba8")
                    v = reference(seed, shape, size, name, srgb_space)
                    want = resize_ref.quantise(v)
                    assert got.shape == want.shape and (got[..., 3] == 255).all()
                    d = got[..., :3].astype(int) - want[..., :3].astype(int)
                    assert np.abs(d).max() <= 1
                    if (d != 0).any():
                        frac = 255.0 * v + 0.5
                        assert np.abs(frac - np.round(frac))[d != 0].max() < 255 * 1e-4, "u8 mismatch away from a rounding knife-edge"
                    differing += int((d != 0).sum())
                    total += d.size
    print(f"differing bytes: {differing} of {total}")
    assert differing / total < 1e-3


@pytest.mark.parametrize("name", FILTERS)
def test_a_batch_is_its_images_bit_for_bit(engines, name):
    eng = engines(graph="bilinear")
    for (shape, size) in (((7, 9), (3, 4)), ((9, 257), (5, 129)), ((5, 31), (8, 50))):
        px = rgba(77, 2, *shape)
        assert (px[0] != px[1]).any()
        for in_kind, out_kind in (("rgba8", "rgba8"), ("f32", "f32"), ("rgba8", "f32"), ("f32", "rgba8")):
            both = run(eng, px, size, name, False, in_kind, out_kind)
            for i in range(2):
                np.testing.assert_array_equal(both[i], run(eng, px[i:i + 1], size, name, False, in_kind, out_kind)[0])


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("srgb_space", [False, True])
def test_identity_size_returns_the_colour_bytes(engines, name, srgb_space):
    eng = engines(graph="bilinear")
    for shape in ((1, 1), (33, 17), (9, 257), (70, 300)):
        px = rgba(5, 2, *shape)
        got = run(eng, px, shape, name, srgb_space, "rgba8", "rgba8")
        np.testing.assert_array_equal(got[..., :3], px[..., :3])
        assert (got[..., 3] == 255).all()
        host = eng.resize(px, shape, name, srgb_space)
        np.testing.assert_array_equal(host, got)


def test_box_and_triangle_are_the_parameter_free_graphs(engines):
    import rusty_sr_amd as r
    bil = engines(graph="bilinear")
    down = engines(graph="downsample")
    rng = np.random.default_rng(11)
    for shape in ((3, 3), (12, 27), (66, 129)):
        x = rng.random((2,) + shape + (3,), dtype=np.float32)
        got = bil.resize(x, (shape[0] // 3, shape[1] // 3), "box")
        want = down.upscale_f32(x)
        assert got.shape == want.shape and np.abs(got - want).max() < TOL
    for shape in ((1, 1), (5, 2), (40, 70)):
        x = rng.random((2,) + shape + (3,), dtype=np.float32)
        got = bil.resize(x, (3 * shape[0], 3 * shape[1]), "triangle")
        want = bil.upscale_f32(x)
        assert got.shape == want.shape and np.abs(got - want).max() < TOL
    assert r.Engine.FILTERS["box"] == 0 and r.Engine.FILTERS["lanczos3"] == 3


@pytest.mark.parametrize("factor,graph,precision", [(f, "sr_net", p) for f in (2, 3, 4) for p in ("f32", "split_f16")] + [(3, "bilinear", "f32")])
def test_sized_call_is_the_network_then_the_resampling(engines, factor, graph, precision):
    """Bit for bit: upscale_rgba8_sized_dev == upscale_f32_dev (or the f32 ensemble) on byte / 255, then resize_dev f32 -> RGBA8; the host
    call equals the device call; the same call twice gives the same bytes."""
    import torch
    import rusty_sr_amd as r
    eng = engines(factor, graph)
    if graph == "sr_net":
        eng.set_precision(precision)
    try:
        for (h, w), name in (((9, 11), "lanczos3"), ((40, 70), "catrom")):
            px = np.concatenate([synth_u8(h * w + factor, 1, h, w), rgba(3, 1, h, w)[..., 3:]], axis=-1)
            fh, fw = factor * h, factor * w
            tpx = torch.from_numpy(px).cuda()
            x = torch.from_numpy(r.img_to_data(px)).cuda()
            for members in ((1, 0xFF) if graph == "sr_net" and (h, w) == (9, 11) else (1,)):
                net = eng.upscale_f32_dev(x) if members == 1 else eng.upscale_ensemble_f32_dev(x, members)
                for size in ((max(1, 2 * fh // 3), fw // 2), (fh + 5, 3 * fw // 2)):
                    want = eng.resize_dev(net, size, "rgba8", name).cpu().numpy()
                    got = eng.upscale_rgba8_sized_dev(tpx, size, name, members=members).cpu().numpy()
                    assert got.shape == (1,) + size + (4,)
                    np.testing.assert_array_equal(got, want)
                    np.testing.assert_array_equal(eng.upscale_rgba8_sized_dev(tpx, size, name, members=members).cpu().numpy(), got)
                    np.testing.assert_array_equal(eng.upscale_rgba8_sized(px, size, name, members=members), got)
                    np.testing.assert_array_equal(eng.upscale_rgba8_sized(px[0], size, name, members=members), got[0])
    finally:
        if graph == "sr_net":
            eng.set_precision("f32")


@pytest.mark.parametrize("members", [0x03, 0x05])
@pytest.mark.parametrize("precision", ["f32", "split_f16"])
def test_sized_batch_with_an_ensemble_is_its_images(engines, precision, members):
    """A batch under a mask other than 1 runs the ensemble image by image between the batch's f32 buffers: byte for byte the single-image
    calls (which the test above holds to the primitives).  9 x 7: mask 0x05 runs a transposed member on a shape that is not square."""
    import torch
    eng = engines()
    eng.set_precision(precision)
    try:
        batch, size = rgba(members, 2, 9, 7), (31, 17)
        got = eng.upscale_rgba8_sized(batch, size, members=members)
        dev = eng.upscale_rgba8_sized_dev(torch.from_numpy(batch).cuda(), size, members=members).cpu().numpy()
        assert got.shape == (2, 31, 17, 4) and not np.array_equal(got[0], got[1])
        for i in range(2):
            np.testing.assert_array_equal(got[i], eng.upscale_rgba8_sized(batch[i], size, members=members), err_msg=f"image {i}")
            one = eng.upscale_rgba8_sized_dev(torch.from_numpy(batch[i:i + 1]).cuda(), size, members=members).cpu().numpy()
            np.testing.assert_array_equal(dev[i], one[0], err_msg=f"image {i}, device call")
    finally:
        eng.set_precision("f32")


def offset_view(nbytes, offset):
    """nbytes of device memory `offset` bytes into a larger allocation filled with 0xA5, and the whole allocation."""
    import torch
    whole = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + nbytes], whole


def test_refusals(engines, params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil, down = engines(), engines(graph="bilinear"), engines(graph="downsample")
    h, w, oh, ow = 8, 9, 5, 13
    px = rgba(1, 1, h, w)
    tpx = torch.from_numpy(px).cuda()
    out, whole = offset_view(oh * ow * 12, 16)
    L, INV, BIG = e._L, _lib.SR_E_INVALID, 2**31 - 1
    stream = e._stream_ptr(None, tpx.device)
    p_in, p_out = C.c_void_p(tpx.data_ptr()), C.c_void_p(out.data_ptr())
    U8, F32, LZ = _lib.SR_PIXELS_RGBA8, _lib.SR_PIXELS_F32, _lib.SR_FILTER_LANCZOS3

    def resize(ctx=e._ctx, d_in=p_in, ip=U8, n=1, hh=h, ww=w, d_out=p_out, op=U8, o_h=oh, o_w=ow, flt=LZ, flags=0):
        return L.sr_resize_dev(ctx, d_in, ip, n, hh, ww, d_out, op, o_h, o_w, flt, flags, stream)

    def sized(ctx=e._ctx, d_in=p_in, n=1, hh=h, ww=w, d_out=p_out, o_h=oh, o_w=ow, flt=LZ, flags=0, members=1):
        return L.sr_upscale_rgba8_sized_dev(ctx, d_in, n, hh, ww, d_out, o_h, o_w, flt, flags, members, stream)

    for call in (resize, sized):
        assert call(ctx=None) == INV and call(d_in=None) == INV and call(d_out=None) == INV
        for bad in (dict(n=0), dict(hh=0), dict(ww=0), dict(o_h=0), dict(o_w=0), dict(n=-1), dict(o_h=-3)):
            assert call(**bad) == INV, bad
        assert call(n=BIG, hh=BIG, ww=BIG) == INV and call(n=BIG, o_h=BIG, o_w=BIG) == INV  # byte counts beyond a size_t
        for flt in (-1, 4, 1 << 20):
            assert call(flt=flt) == INV
        for flags in (2, 3, 1 << 31):
            assert call(flags=flags) == INV
        assert call(d_out=p_in) == INV  # in place
        for off in (1, 2, 3):
            assert call(d_out=C.c_void_p(out.data_ptr() + off)) == INV
            assert call(d_in=C.c_void_p(tpx.data_ptr() + off)) == INV
    for kind in (-1, 2, 7):
        assert resize(ip=kind) == INV and resize(op=kind) == INV
    assert sized(ctx=down._ctx) == INV
    for members in (0, 256, 1 << 20):
        assert sized(members=members) == INV
    for members in (0, 3, 0xFF, 256):
        assert sized(ctx=bil._ctx, members=members) == INV
    assert sized(hh=BIG // 2) == INV  # factor x h beyond an int
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    # the host forms, through the binding
    host_out = np.full((oh, ow, 4), 0xA5, np.uint8)
    for call in (lambda: e.resize(px, (oh, ow), 4, out=host_out), lambda: e.resize(px, (0, ow)), lambda: e.resize(px, (oh, -1)),
                 lambda: e.upscale_rgba8_sized(px, (oh, ow), members=0, out=host_out), lambda: e.upscale_rgba8_sized(px, (oh, ow), 9, out=host_out),
                 lambda: bil.upscale_rgba8_sized(px, (oh, ow), members=3, out=host_out), lambda: down.upscale_rgba8_sized(px, (oh, ow), out=host_out),
                 lambda: e.upscale_rgba8_sized_dev(tpx, (0, 4))):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    assert (host_out == 0xA5).all()
    # a shape no device can hold is SR_E_NOMEM before anything is launched, and the context still serves
    assert resize(hh=400000, ww=400000, o_h=300000, o_w=300000) == _lib.SR_E_NOMEM
    assert sized(hh=400000, ww=400000) == _lib.SR_E_NOMEM
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    fresh = r.Engine(params["imagenet"])
    np.testing.assert_array_equal(e.upscale_rgba8_sized(px, (oh, ow)), fresh.upscale_rgba8_sized(px, (oh, ow)))
    np.testing.assert_array_equal(e.resize(px, (oh, ow)), fresh.resize(px, (oh, ow)))
    fresh.close()


def test_other_stream_and_offset_views(engines):
    """The _dev calls on a non-default torch stream, the output and the input 4 bytes into a larger buffer: the guard bytes either side stay."""
    import torch
    e = engines()
    (h, w), (oh, ow) = (9, 11), (20, 7)
    px = rgba(9, 1, h, w)
    tpx = torch.from_numpy(px).cuda()
    want = e.resize_dev(tpx, (oh, ow)).cpu().numpy()
    want_sized = e.upscale_rgba8_sized_dev(tpx, (oh, ow)).cpu().numpy()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for offset in (4, 12):
        src, src_whole = offset_view(h * w * 4, offset)
        src.copy_(tpx.reshape(-1))
        src_img = src.view(1, h, w, 4)
        side.wait_stream(torch.cuda.current_stream())
        for fn, ref in ((e.resize_dev, want), (e.upscale_rgba8_sized_dev, want_sized)):
            dst, dst_whole = offset_view(oh * ow * 4, offset)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                fn(src_img, (oh, ow), out=dst.view(1, oh, ow, 4))
                fn(src_img, (oh, ow), out=dst.view(1, oh, ow, 4), stream=side)
            side.synchronize()
            np.testing.assert_array_equal(dst.view(1, oh, ow, 4).cpu().numpy(), ref)
            guard = dst_whole.cpu().numpy()
            assert (guard[:offset] == 0xA5).all() and (guard[offset + oh * ow * 4:] == 0xA5).all()
        guard = src_whole.cpu().numpy()
        assert (guard[:offset] == 0xA5).all() and (guard[offset + h * w * 4:] == 0xA5).all()
        np.testing.assert_array_equal(src.cpu().numpy(), px.reshape(-1))


def test_cli_writes_the_asked_size(engines, tmp_path):
    from PIL import Image
    from rusty_sr_amd.build import build_host
    build_host()
    e = engines()
    src = os.path.join(ROOT, "tests", "golden", "butterfly_lr.png")
    px = load_png("butterfly_lr.png")
    if px.shape[-1] == 3:
        px = np.concatenate([px, np.full(px.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    h, w = px.shape[:2]
    out = tmp_path / "out.png"

    def run_cli(*args, head="Upscaling using imagenet neural net parameters..."):
        res = subprocess.run([CLI, src, str(out), *args], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stderr
        assert res.stdout == head + " Writing file... Done\n"
        if "--timing" in args:  # the sized call times itself: the network and the three launches of the resampling between the copies
            kernels, h2d, d2h = map(float, re.search(r"kernels ([\d.]+) ms, h2d ([\d.]+) ms, d2h ([\d.]+) ms", res.stderr).groups())
            assert kernels > 0 and h2d > 0 and d2h > 0, res.stderr
        got = np.array(Image.open(out).convert("RGBA"))
        os.remove(out)
        return got

    got = run_cli("--size", "500x333")
    assert got.shape == (333, 500, 4)
    np.testing.assert_array_equal(got, e.upscale_rgba8_sized(px, (333, 500)))
    got = run_cli("--scale", "1.5", "--timing")
    assert got.shape == resize_ref.scaled_size(h, w, 1.5) + (4,)
    np.testing.assert_array_equal(got, e.upscale_rgba8_sized(px, got.shape[:2]))
    got = run_cli("--scale=2", "--filter", "catrom", "--resize-space", "srgb", "--ensemble", "2")
    np.testing.assert_array_equal(got, e.upscale_rgba8_sized(px, (2 * h, 2 * w), "catrom", srgb_space=True, members=0x03))
    got = run_cli("--size", "100x80", "-p", "bilinear", "--filter", "box", head="Upscaling using bilinear interpolation...")
    np.testing.assert_array_equal(got, engines(graph="bilinear").upscale_rgba8_sized(px, (80, 100), "box"))
