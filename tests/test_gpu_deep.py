"""Deep colour on the GPU (include/srhip.h "Deep colour"): both conversion kernels against tests/deep_ref.py bit for bit at every
count, offset and form, each composed call against its device calls chained by hand and against the oracle, what the feature is for
(a gradient inside one 8-bit level), the host calls, the refusals and the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deep_ref
import oracle
import param_families
from conftest import load_png, synth_u8

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
ALL8 = 0xFF
GUARD = 64
# The library against deep_ref.quantise(oracle.forward(params, deep_ref.to_f32(x))), in levels: the project's own bar before
# quantisation is 1e-4 (tests/test_gpu_parity.py), 6.55 levels of 1 / 65535, and the two roundings may fall either side of a step.
ORACLE_LEVELS = 7


def span():
    from rusty_sr_amd import _lib
    return _lib.SR_DEEP_SPAN


def counts():
    """Pixel counts either side of what the kernels cut the run by: a lane's group of 8 pixels and a workgroup's SR_DEEP_SPAN pixels
    (the kernels do not loop: a workgroup takes one span); (n, h, w) with n = 2 among them -- the batch is one run of pixels."""
    s = span()
    return ((1, 1, 1), (1, 1, 7), (1, 1, 8), (1, 1, 9), (1, 1, s - 1), (1, 1, s), (1, 1, s + 1), (2, 3, s // 2 + 5))


@pytest.fixture(scope="module")
def engines():
    import rusty_sr_amd as r
    made = {}

    def get(precision="f32", factor=3, graph="sr_net"):
        k = (precision, factor, graph)
        if k not in made:
            if graph != "sr_net":
                made[k] = r.Engine(graph=graph)
            else:
                p = param_families.weights("imagenet" if factor == 3 else "bundled_scale", factor)
                made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


class Guarded:
    """`nbytes` on the GPU whose first byte lies `offset` bytes past a 16-byte boundary, with GUARD bytes of 0xA5 either side."""

    def __init__(self, nbytes, offset, data=None):
        import torch
        self.whole = torch.full((nbytes + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.lo, self.n = GUARD + offset, nbytes
        if data is not None:
            self.whole[self.lo:self.lo + nbytes] = torch.from_numpy(np.frombuffer(data.tobytes(), np.uint8).copy()).cuda()
        self.ptr = C.c_void_p(self.whole.data_ptr() + self.lo)

    def bytes(self):
        return self.whole[self.lo:self.lo + self.n].cpu().numpy().tobytes()

    def guards_intact(self):
        return bool((self.whole[:self.lo] == 0xA5).all() and (self.whole[self.lo + self.n:] == 0xA5).all())


def run_to_f32(e, px, src_off, dst_off):
    import torch
    n, h, w, c = px.shape
    src, dst = Guarded(px.nbytes, src_off, px), Guarded(n * h * w * 12, dst_off)
    rc = e._L.sr_u16_to_f32_dev(e._ctx, src.ptr, c, n, h, w, dst.ptr, e._stream_ptr(None, "cuda:0"))
    form = [o.get("form") for o in e.last_plan()["ops"]]
    torch.cuda.synchronize()
    assert rc == 0 and src.guards_intact() and dst.guards_intact(), (rc, src_off, dst_off)
    return np.frombuffer(dst.bytes(), np.float32).reshape(n, h, w, 3), form


def run_to_u16(e, x, oc, src_off, dst_off):
    import torch
    n, h, w, _ = x.shape
    src, dst = Guarded(x.nbytes, src_off, x), Guarded(n * h * w * oc * 2, dst_off)
    rc = e._L.sr_f32_to_u16_dev(e._ctx, src.ptr, n, h, w, dst.ptr, oc, e._stream_ptr(None, "cuda:0"))
    form = [o.get("form") for o in e.last_plan()["ops"]]
    torch.cuda.synchronize()
    assert rc == 0 and src.guards_intact() and dst.guards_intact(), (rc, src_off, dst_off)
    return np.frombuffer(dst.bytes(), np.uint16).reshape(n, h, w, oc), form


def form_of(in_off, out_off):
    return {(True, True): "wide", (True, False): "wide_in", (False, True): "wide_out", (False, False): "narrow"}[(in_off == 0, out_off == 0)]


# ---- 1. the two launches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ic", [1, 2, 3, 4])
def test_u16_to_f32_is_the_restatement(engines, ic):
    e = engines()
    rng = np.random.default_rng(ic)
    for (n, h, w) in counts():
        px = rng.integers(0, 65536, (n, h, w, ic), dtype=np.uint16)
        want = deep_ref.to_f32(px)
        for src_off in (0, 2):
            for dst_off in (0, 4, 8, 12):
                got, form = run_to_f32(e, px, src_off, dst_off)
                assert got.tobytes() == want.tobytes(), (n, h, w, src_off, dst_off)
                assert form == [form_of(src_off, dst_off)]
    # every one of the 65536 levels, in both forms of the source side
    npx = 65536 + 11
    px = rng.integers(0, 65536, (1, 1, npx, ic), dtype=np.uint16)
    px[0, 0, :, 0] = (np.arange(npx) * 40503 % 65536).astype(np.uint16)      # (an odd multiplier: a permutation of the levels)
    if ic >= 3:
        px[0, 0, :, 1] = (np.arange(npx) + 7).astype(np.uint16)
        px[0, 0, :, 2] = (65535 - np.arange(npx) % 65536).astype(np.uint16)
    assert len(np.unique(px[..., 0])) == 65536
    want = deep_ref.to_f32(px)
    for src_off, dst_off in ((0, 0), (2, 4)):
        got, _ = run_to_f32(e, px, src_off, dst_off)
        assert got.tobytes() == want.tobytes(), (src_off, dst_off)


def special_values():
    """Every level k / 65535, every tie (k + 0.5) / 65535 with its two f32 neighbours, -0.0, negatives, values above 1, the infinities,
    NaN, denormals, and seeded noise in [-0.1, 1.1]; a whole number of pixels."""
    F = np.float32
    k = np.arange(65536, dtype=np.float32)
    levels = k / F(65535.0)
    ties = ((k.astype(np.float64) + 0.5) / 65535.0).astype(F)
    odd = np.array([-0.0, 0.0, -1e-3, -1.0, -1e30, 1.0, 1.0000001, 1.5, 3e38, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 1.1754942e-38,
                    7.62951e-06, 0.49999997, 0.5, 0.99999994], dtype=F)
    noise = (np.random.default_rng(5).random(4001, dtype=F) * F(1.2) - F(0.1)).astype(F)
    v = np.concatenate([levels, ties, np.nextafter(ties, F(-1)), np.nextafter(ties, F(2)), odd, noise])
    v = np.concatenate([v, np.zeros((-len(v)) % 3, F)])
    return levels, v.reshape(1, 1, -1, 3)


@pytest.mark.parametrize("oc", [1, 3, 4])
def test_f32_to_u16_is_the_restatement(engines, oc):
    e = engines()
    rng = np.random.default_rng(10 + oc)
    levels, special = special_values()
    for (n, h, w) in counts():
        x = (rng.random((n, h, w, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
        flat = x.reshape(-1)
        flat[::5] = special.reshape(-1)[rng.integers(0, special.size, len(flat[::5]))]
        want = deep_ref.quantise(x, oc)
        for src_off in (0, 4, 8, 12):
            for dst_off in (0, 2):
                got, form = run_to_u16(e, x, oc, src_off, dst_off)
                assert got.tobytes() == want.tobytes(), (n, h, w, src_off, dst_off)
                assert form == [form_of(src_off, dst_off)]
    want = deep_ref.quantise(special, oc)
    for src_off, dst_off in ((0, 0), (4, 2)):
        got, _ = run_to_u16(e, special, oc, src_off, dst_off)
        assert got.tobytes() == want.tobytes(), (src_off, dst_off)
    # every k / 65535 returns k: as a colour sample, and as the grey mean of a grey pixel
    x = np.repeat(levels[:, None], 3, axis=1).reshape(1, 1, 65536, 3)
    for src_off, dst_off in ((0, 0), (8, 2)):
        got, _ = run_to_u16(e, x, oc, src_off, dst_off)
        for ch in range(min(oc, 3)):
            assert (got[0, 0, :, ch] == np.arange(65536)).all(), (ch, src_off)
        assert oc != 4 or (got[..., 3] == 65535).all()


# ---- 2. the composed calls -----------------------------------------------------------------------------------------------------------
def smooth_u16(seed, n, h, w, c=3):
    """A smooth 16-bit picture: synth_u8's pixels promoted, with seeded low bytes; c = 1 grey, 2 / 4 with a random alpha channel."""
    rng = np.random.default_rng(seed)
    base = synth_u8(seed, n, h, w).astype(np.int64) * 257 + rng.integers(-128, 129, (n, h, w, 3))
    px = np.clip(base, 0, 65535).astype(np.uint16)
    if c <= 2:
        px = px[..., :1]
    if c in (2, 4):
        px = np.concatenate([px, rng.integers(0, 65536, (n, h, w, 1), dtype=np.uint16)], axis=-1)
    return np.ascontiguousarray(px)


def chained(e, px, oc, members=1, border=None, sized=None):
    import torch
    x = e.u16_to_f32_dev(torch.from_numpy(px).cuda())
    if border is not None:
        net = e.upscale_f32_border_dev(x, border[0], border[1], members)
    else:
        net = e.upscale_f32_dev(x) if members == 1 else e.upscale_ensemble_f32_dev(x, members=members)
        if sized is not None:
            net = e.resize_dev(net, sized[0], "f32", sized[1], sized[2])
    out = e.f32_to_u16_dev(net, oc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_plain_call_is_its_three_device_calls(engines, precision, factor):
    import torch
    e = engines(precision, factor)
    for (n, h, w, ic, oc) in ((1, 8, 8, 3, 3), (2, 13, 10, 4, 4), (1, 33, 17, 1, 1), (2, 13, 10, 2, 3)):
        px = smooth_u16(factor * 100 + h + ic, n, h, w, ic)
        for members in (1, 0x03, ALL8):
            want = chained(e, px, oc, members)
            assert want.shape == (n, factor * h, factor * w, oc) and want.min() != want.max()
            dev = e.upscale_u16_dev(torch.from_numpy(px).cuda(), oc, members)
            ops = [(o["name"], o.get("form")) for o in e.last_plan()["ops"]]
            torch.cuda.synchronize()
            assert dev.cpu().numpy().tobytes() == want.tobytes(), (h, w, members, "dev")
            assert ops[0] == ("u16_to_f32", "wide") and ops[-1] == ("f32_to_u16", "wide")
            assert e.upscale_u16(px, oc, members).tobytes() == want.tobytes(), (h, w, members, "host")
        if n == 2:   # the images of a batch do not see each other
            assert e.upscale_u16(px[1], oc).tobytes() == chained(e, px, oc)[1].tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_border_call_is_its_device_calls(engines, precision):
    import torch
    for factor, cases in ((3, [(m, p) for m in (1, 2, 3) for p in (7, 8)]), (2, [(1, 8)])):
        e = engines(precision, factor)
        for (n, h, w, ic, oc) in ((2, 13, 10, 3, 3), (1, 8, 8, 1, 1)):
            px = smooth_u16(31 + h, n, h, w, ic)
            for mode, pad in cases:
                for members in ((1, 0x03) if (mode, pad) != (1, 8) else (1, 0x03, ALL8)):
                    want = chained(e, px, oc, members, border=(mode, pad))
                    dev = e.upscale_u16_border_dev(torch.from_numpy(px).cuda(), mode, pad, members, oc)
                    torch.cuda.synchronize()
                    assert dev.cpu().numpy().tobytes() == want.tobytes(), (mode, pad, members, "dev")
                    assert e.upscale_u16_border(px, mode, pad, members, oc).tobytes() == want.tobytes(), (mode, pad, members, "host")
            assert chained(e, px, oc, border=(1, 8)).tobytes() != chained(e, px, oc).tobytes()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sized_call_is_its_device_calls(engines, precision):
    import torch
    e = engines(precision)
    for filt, size, srgb in (("box", (20, 41), False), ("triangle", (31, 29), False), ("catrom", (64, 50), True), ("lanczos3", (17, 23), False)):
        for (n, h, w, ic, oc) in ((2, 13, 10, 3, 3), (1, 33, 17, 2, 1)):
            px = smooth_u16(57 + h, n, h, w, ic)
            for members in (1, 0x03):
                want = chained(e, px, oc, members, sized=(size, filt, srgb))
                assert want.shape == (n,) + size + (oc,)
                dev = e.upscale_u16_sized_dev(torch.from_numpy(px).cuda(), size, filt, srgb, members, oc)
                torch.cuda.synchronize()
                assert dev.cpu().numpy().tobytes() == want.tobytes(), (filt, members, "dev")
                assert e.upscale_u16_sized(px, size, filt, srgb, members, oc).tobytes() == want.tobytes(), (filt, members, "host")


def test_parameter_free_graphs(engines):
    """-p bilinear takes all three calls; the downsample graph the plain one, and pools in linear light."""
    import rusty_sr_amd as r
    bil, down = engines(graph="bilinear"), engines(graph="downsample")
    px = smooth_u16(77, 2, 13, 10, 3)
    assert bil.upscale_u16(px).tobytes() == chained(bil, px, 3).tobytes()
    assert bil.upscale_u16_border(px, "mirror", 7).tobytes() == chained(bil, px, 3, border=(3, 7)).tobytes()
    assert bil.upscale_u16_sized(px, (20, 21), "catrom").tobytes() == chained(bil, px, 3, sized=((20, 21), "catrom", False)).tobytes()
    got = down.upscale_u16(px, 1)
    assert got.shape == (2, 4, 3, 1) and got.tobytes() == chained(down, px, 1).tobytes()
    want = deep_ref.quantise(oracle.downsample(deep_ref.to_f32(px)))
    assert np.abs(down.upscale_u16(px).astype(int) - want.astype(int)).max() <= ORACLE_LEVELS
    for call in (lambda: down.upscale_u16_border(px), lambda: down.upscale_u16_sized(px, (5, 5)), lambda: down.upscale_u16(px[:, :2])):
        with pytest.raises(r.SrError):
            call()


# ---- 3. against the oracle -----------------------------------------------------------------------------------------------------------
def oracle_images():
    """A cut of butterfly_lr.png promoted to 16 bits with seeded low bytes, and a smooth seeded picture."""
    rng = np.random.default_rng(2031)
    cut = load_png("butterfly_lr.png")[40:88, 30:94, :3].astype(np.int64) * 257 + rng.integers(0, 257, (48, 64, 3))
    return (("butterfly", np.clip(cut, 0, 65535).astype(np.uint16)), ("smooth", smooth_u16(2032, 1, 48, 64)[0]))


_ORACLE = {}


def oracle_u16(name, px, oc=3):
    if (name, oc) not in _ORACLE:
        _ORACLE[(name, oc)] = deep_ref.quantise(oracle.forward(param_families.weights("imagenet", 3), deep_ref.to_f32(px)[None])[0], oc)
    return _ORACLE[(name, oc)]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_oracle(engines, precision):
    e = engines(precision)
    for name, px in oracle_images():
        for oc in (3, 1):
            want = oracle_u16(name, px, oc)
            got = e.upscale_u16(px, oc)
            d = np.abs(got.astype(int) - want.astype(int))
            print(f"{name}, {precision}, {oc} channels: max level diff = {d.max()}, share differing = {(d != 0).mean():.3g}")
            assert got.shape == want.shape and d.max() <= ORACLE_LEVELS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_gradient_inside_one_8_bit_level_survives(engines, precision):
    """Samples 0x8000 .. 0x80FF: the 8-bit path sees one constant image (high byte 0x80) and answers with one; the 16-bit path keeps
    the gradient and stays within the oracle bound on the exact input."""
    e = engines(precision)
    h, w = 24, 32
    ramp = (0x8000 + (np.arange(w)[None, :] * 255 // (w - 1) + np.arange(h)[:, None] * 0) % 256).astype(np.uint16)
    px = np.repeat(ramp[:, :, None], 3, axis=2)
    px[:, :, 1] = 0x8000 + (np.arange(h)[:, None] * 255 // (h - 1) + np.zeros(w, int)[None, :])
    assert px.min() == 0x8000 and px.max() == 0x80FF
    high = np.concatenate([(px >> 8).astype(np.uint8), np.full((h, w, 1), 255, np.uint8)], axis=2)
    assert len(np.unique(high[..., :3])) == 1
    flat8 = e.upscale_rgba8(high)[..., :3]
    inner8 = flat8[24:-24, 24:-24]
    assert all(len(np.unique(inner8[..., ch])) == 1 for ch in range(3))     # (away from the zero-padded edge the 8-bit answer is flat)
    got = e.upscale_u16(px)
    inner = got[24:-24, 24:-24]
    assert len(np.unique(inner[..., 0])) > 16 and len(np.unique(inner[..., 1])) > 16   # not constant: the gradient is there
    want = deep_ref.quantise(oracle.forward(param_families.weights("imagenet", 3), deep_ref.to_f32(px)[None])[0])
    d = np.abs(got.astype(int) - want.astype(int))
    print(f"gradient, {precision}: max level diff = {d.max()}")
    assert d.max() <= ORACLE_LEVELS


# ---- 4. host and device calls --------------------------------------------------------------------------------------------------------
def test_two_contexts_give_the_same_bits_and_timing_works():
    import rusty_sr_amd as r
    p = param_families.weights("imagenet", 3)
    px = smooth_u16(91, 2, 13, 10, 4)
    a, b = r.Engine(p), r.Engine(p)
    first = a.upscale_u16(px, 4, ALL8)
    assert first.tobytes() == b.upscale_u16(px, 4, ALL8).tobytes() == a.upscale_u16(px, 4, ALL8).tobytes()
    assert (first[..., 3] == 65535).all()
    a.set_profiling(True)
    assert a.upscale_u16(px, 4).tobytes() == b.upscale_u16(px, 4).tobytes()
    t = a.last_timing()
    assert t["total_ms"] > 0 and t["h2d_ms"] > 0 and t["d2h_ms"] > 0
    grey = a.upscale_u16(px[0, :, :, 0])
    assert grey.shape == (39, 30) and grey.dtype == np.uint16
    a.close()
    b.close()


def test_split_half_host_call_recomputes_in_f32_when_a_value_leaves_the_domain():
    """tests/domain_cases.py's wiring, as tests/test_gpu_video.py uses it: channel 5 of the first layer leaves the split-half domain on
    any image.  The device call raises the word; the host call equals the exact-f32 call's samples."""
    import torch
    import domain_cases
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    p = domain_cases.wired("f", 5, 1.0)
    domain_cases._view(p, 3, "f_bias")[5] = 7e4
    px = smooth_u16(93, 1, 13, 10)
    exact = r.Engine(p, precision="f32")
    want = exact.upscale_u16(px)
    exact.close()
    e = r.Engine(p, precision="split_f16")
    e.upscale_u16_dev(torch.from_numpy(px).cuda())
    torch.cuda.synchronize()
    assert e._L.sr_check_domain(e._ctx) == _lib.SR_E_DOMAIN
    assert e.upscale_u16(px).tobytes() == want.tobytes()
    assert e.upscale_u16_border(px, "wrap").shape == want.shape and e.precision == "split_f16"
    e.close()


def test_refusals(engines):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil, down = engines(), engines(graph="bilinear"), engines(graph="downsample")
    h, w, f = 6, 10, 3
    px = smooth_u16(95, 1, h, w, 3)
    src = Guarded(px.nbytes, 0, px)
    rgb = torch.zeros((1, f * h, f * w, 3), dtype=torch.float32, device="cuda")
    out = Guarded(f * h * f * w * 12, 0)
    L, INV = e._L, _lib.SR_E_INVALID
    stream = e._stream_ptr(None, "cuda:0")
    p_in, p_rgb, p_out = src.ptr, C.c_void_p(rgb.data_ptr()), out.ptr

    def up(ctx=e._ctx, a=p_in, ic=3, n=1, hh=h, ww=w, b=p_out, oc=3, members=1):
        return L.sr_upscale_u16_dev(ctx, a, ic, n, hh, ww, b, oc, members, stream)

    def border(ctx=e._ctx, a=p_in, ic=3, n=1, hh=h, ww=w, b=p_out, oc=3, members=1, mode=1, pad=8):
        return L.sr_upscale_u16_border_dev(ctx, a, ic, n, hh, ww, b, oc, mode, pad, members, stream)

    def sized(ctx=e._ctx, a=p_in, ic=3, n=1, hh=h, ww=w, b=p_out, oc=3, members=1, oh=11, ow=13, filt=3, flags=0):
        return L.sr_upscale_u16_sized_dev(ctx, a, ic, n, hh, ww, b, oc, oh, ow, filt, flags, members, stream)

    def to_f32(ctx=e._ctx, a=p_in, ic=3, n=1, hh=h, ww=w, b=p_out):
        return L.sr_u16_to_f32_dev(ctx, a, ic, n, hh, ww, b, stream)

    def to_u16(ctx=e._ctx, a=p_rgb, n=1, hh=h, ww=w, b=p_out, oc=3):
        return L.sr_f32_to_u16_dev(ctx, a, n, hh, ww, b, oc, stream)

    odd = lambda p, k=1: C.c_void_p(p.value + k)
    for call in (up, border, sized, to_f32, to_u16):
        assert call(a=None) == INV and call(b=None) == INV, call.__name__
        for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (2 ** 30, 2 ** 30, 2 ** 30)):
            assert call(n=n, hh=hh, ww=ww) == INV, (call.__name__, n, hh, ww)
    for call in (up, border, sized, to_f32):
        assert call(a=odd(p_in)) == INV and call(ic=0) == INV and call(ic=5) == INV and call(ic=-1) == INV, call.__name__
    for call in (up, border, sized, to_u16):
        assert call(b=odd(p_out)) == INV and call(oc=0) == INV and call(oc=2) == INV and call(oc=5) == INV, call.__name__
    for call in (up, border, sized):
        for members in (0, 256, 1 << 20):
            assert call(members=members) == INV, (call.__name__, members)
        for members in (3, ALL8):
            assert call(ctx=bil._ctx, members=members) == INV
        assert call(hh=2 ** 30) == INV and call(ww=2 ** 30) == INV
    for k in (1, 2, 3):                                                   # the f32 side is dword-aligned
        assert to_f32(b=odd(p_out, k)) == INV and to_u16(a=odd(p_rgb, k)) == INV
    assert to_f32(b=p_in) == INV and to_u16(a=p_rgb, b=p_rgb) == INV       # d_in == d_out
    assert up(ctx=down._ctx, members=3) == INV and up(ctx=down._ctx, hh=2) == INV
    assert border(ctx=down._ctx) == INV and sized(ctx=down._ctx) == INV
    for mode, pad in ((0, 8), (4, 8), (1, 6), (1, 33)):
        assert border(mode=mode, pad=pad) == INV
    assert sized(oh=0) == INV and sized(ow=-1) == INV and sized(filt=4) == INV and sized(filt=-1) == INV and sized(flags=2) == INV
    torch.cuda.synchronize()
    assert out.bytes() == b"\xa5" * out.n and out.guards_intact()
    # a shape whose workspace no device holds is SR_E_NOMEM by arithmetic; the context still serves, and any context converts
    assert up(hh=150000, ww=150000) == _lib.SR_E_NOMEM
    want = chained(e, px, 3)
    assert e.upscale_u16(px).tobytes() == want.tobytes()
    assert to_f32(ctx=down._ctx) == _lib.SR_OK
    torch.cuda.synchronize()
    assert out.bytes()[:h * w * 12] == deep_ref.to_f32(px).tobytes()
    # the host forms, through the binding
    for call in (lambda: e.upscale_u16(px, 2), lambda: e.upscale_u16(px, members=0), lambda: bil.upscale_u16(px, members=3),
                 lambda: e.upscale_u16_border(px, 5), lambda: e.upscale_u16_sized(px, (0, 4))):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    with pytest.raises(ValueError):
        e.upscale_u16(np.zeros((4, 4, 5), np.uint16))


# ---- 5. the CLI ----------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rusty_sr_amd", "bin", "rusty_sr")


def cli(*args):
    return subprocess.run([CLI, *map(str, args)], capture_output=True, timeout=120)


def test_cli_depth_16(engines, tmp_path):
    from rusty_sr_amd.build import build_host
    from test_deep_cpu import read_png, write_png16
    build_host()
    e = engines()
    rgb, grey = smooth_u16(401, 1, 13, 10)[0], smooth_u16(402, 1, 13, 10, 1)[0]
    src, gsrc, out = tmp_path / "rgb16.png", tmp_path / "grey16.png", tmp_path / "out.png"
    src.write_bytes(write_png16(rgb, 2))
    gsrc.write_bytes(write_png16(grey, 0, interlace=True))
    # RGB16 in, the library's samples out; --timing names the depth
    res = cli("--depth", "16", "--timing", src, out)
    assert res.returncode == 0, res.stderr
    got, depth, ctype = read_png(out.read_bytes())
    assert depth == 16 and ctype == 2 and got.tobytes() == e.upscale_u16(rgb).tobytes()
    assert b"16 bits, 3 -> 3 channels" in res.stderr
    # grey16 in, grey16 out; a .ppm takes RGB
    res = cli("--depth", "16", gsrc, out)
    assert res.returncode == 0, res.stderr
    got, depth, ctype = read_png(out.read_bytes())
    assert depth == 16 and ctype == 0 and got.tobytes() == e.upscale_u16(grey, 1).tobytes()
    ppm = tmp_path / "out.ppm"
    res = cli("--depth=16", gsrc, ppm)
    assert res.returncode == 0, res.stderr
    data = ppm.read_bytes()
    head = b"P6\n30 39\n65535\n"
    assert data.startswith(head) and np.frombuffer(data[len(head):], ">u2").astype(np.uint16).tobytes() == e.upscale_u16(grey, 3).tobytes()
    # auto: 16 for a 16-bit file and a .png output, the bytes of the run without the flag for an 8-bit file
    res = cli("--depth", "auto", src, out)
    assert res.returncode == 0 and read_png(out.read_bytes())[0].tobytes() == e.upscale_u16(rgb).tobytes(), res.stderr
    from PIL import Image
    src8, plain, auto = tmp_path / "rgb8.png", tmp_path / "plain.png", tmp_path / "auto.png"
    Image.fromarray((rgb >> 8).astype(np.uint8)).save(src8)
    assert cli(src8, plain).returncode == 0 and cli("--depth", "auto", src8, auto).returncode == 0
    assert plain.read_bytes() == auto.read_bytes()
    # one run each with -d, --border and --size (with --filter and --ensemble)
    down = engines(graph="downsample")
    res = cli("--depth", "16", "-d", src, out)
    assert res.returncode == 0 and read_png(out.read_bytes())[0].tobytes() == down.upscale_u16(rgb).tobytes(), res.stderr
    res = cli("--depth", "16", "--border", "wrap", "--border-pad", "7", src, out)
    assert res.returncode == 0 and read_png(out.read_bytes())[0].tobytes() == e.upscale_u16_border(rgb, "wrap", 7).tobytes(), res.stderr
    res = cli("--depth", "16", "--size", "23x17", "--filter", "catrom", "--ensemble", "2", src, out)
    assert res.returncode == 0, res.stderr
    assert read_png(out.read_bytes())[0].tobytes() == e.upscale_u16_sized(rgb, (17, 23), "catrom", members=0x03).tobytes()
