"""The video path on the GPU (include/srhip.h "Video"): both conversion kernels against tests/yuv_ref.py byte for byte and bit for bit on
every grid cell, the composed call against its three device calls chained and against the oracle, the frame stream against the
synchronous call frame by frame, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import yuv_ref
from conftest import load_png, synth_u8
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
FORMS = (("420", "center"), ("420", "left"), ("444", "center"))
FORM_NAME = {("420", "center"): "420center", ("420", "left"): "420left", ("444", "center"): "444"}
SMALL = ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (16, 12), (17, 13))
OFFSETS = (0, 1, 2, 3, 5, 8, 13, 15)   # where a frame begins within a 16-byte group: what a run moves at once (its head and tail are ragged)
ALL8 = 0xFF


def span():
    from rusty_sr_amd import _lib
    return _lib.SR_YUV_SPAN


def wide_shapes():
    """Widths either side of what the kernels cut a row by -- a thread's 4 columns (two chroma samples), a workgroup's SR_YUV_SPAN
    columns -- at 3 and 5 rows: two and three block rows, the last ragged, so that the first, an interior and the last block of both
    grid axes run (the third block column at 2 SR_YUV_SPAN + 1)."""
    s = span()
    return ((3, s - 1), (3, s), (3, s + 1), (3, s + 2), (3, s + 5), (5, 2 * s + 1))


def fmt_of(sub, siting, matrix, range_):
    from rusty_sr_amd import YuvFormat
    return YuvFormat.named(sub, siting, matrix, range_)


def cells(n, h, w):
    return {"n": n, "bx": -(-w // span()), "by": -(-h // 2)}


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


def byte_view(nbytes, offset, fill=0xA5):
    """`nbytes` u8 on the GPU whose first byte lies `offset` bytes into a 16-byte aligned allocation filled with `fill`; and the whole."""
    import torch
    whole = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
    assert whole.data_ptr() % 16 == 0
    return whole[offset:offset + nbytes], whole


def guards_intact(whole, offset, nbytes):
    return bool((whole[:offset] == 0xA5).all() and (whole[offset + nbytes:] == 0xA5).all())


def random_frames(rng, sub, n, h, w):
    """Any byte, 0 and 255 and the codes outside the limited range among them."""
    f = rng.integers(0, 256, (n, yuv_ref.frame_bytes(sub, h, w)), dtype=np.uint8)
    f.reshape(-1)[::7] = 0
    f.reshape(-1)[3::11] = 255
    return f


def random_rgb(rng, n, h, w):
    """f32 in [-2, 3]; +-1e30, the infinities and NaN sprinkled in; grey 0.5 pixels, whose luma sits on a rounding tie (125.5, 127.5)."""
    x = (rng.random((n, h, w, 3), dtype=np.float32) * np.float32(5.0) - np.float32(2.0)).astype(np.float32)
    flat = x.reshape(-1, 3)
    k = len(flat)
    flat[rng.integers(0, k, max(1, k // 9))] = np.float32(0.5)
    flat[rng.integers(0, k, max(1, k // 13))] = rng.random(3, dtype=np.float32)   # in-range pixels too
    vals = x.reshape(-1)
    for i, v in enumerate((1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, 1.0)):
        vals[rng.integers(0, vals.size, max(1, vals.size // 40))] = np.float32(v)
    return x


# ---- 1. the two launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_", yuv_ref.RANGES)
@pytest.mark.parametrize("matrix", tuple(yuv_ref.MATRICES))
@pytest.mark.parametrize("form", FORMS, ids=lambda f: FORM_NAME[f])
def test_conversions_are_the_restatement(engines, form, matrix, range_):
    """Every small shape at n = 1 and 2 with the frames at the byte offsets OFFSETS of a 16-byte group (in and out rotate against each
    other), the wide shapes at n = 2: the f32 RGB equals yuv_ref bit for bit, the frames byte for byte, the bytes around the outputs stay, and the
    recorded op names the grid the shape gives."""
    import torch
    e = engines()
    sub, siting = form
    fmt = fmt_of(sub, siting, matrix, range_)
    rng = np.random.default_rng(sum(map(ord, sub + siting + matrix + range_)))
    runs = [(n, h, w, i) for (h, w) in SMALL for n in (1, 2) for i in range(len(OFFSETS))] + [(2, h, w, w + h) for (h, w) in wide_shapes()]
    for n, h, w, i in runs:
        off = OFFSETS[i % len(OFFSETS)]
        fb = yuv_ref.frame_bytes(sub, h, w)
        # YCbCr -> RGB
        frames = random_frames(rng, sub, n, h, w)
        src, _ = byte_view(n * fb, off)
        src.copy_(torch.from_numpy(frames.reshape(-1)))
        dst, whole = byte_view(n * h * w * 12, 4 * off)
        out = dst.view(torch.float32).view(n, h, w, 3)
        assert e.yuv_to_rgb_dev(src.view(n, fb), fmt, h, w, out=out) is out
        op = e.last_plan()["ops"]
        torch.cuda.synchronize()
        want = np.stack([yuv_ref.yuv_to_rgb(frames[i], h, w, sub, siting, matrix, range_) for i in range(n)])
        assert out.cpu().numpy().tobytes() == want.tobytes(), ("to rgb", n, h, w, off)
        assert guards_intact(whole, 4 * off, n * h * w * 12), ("to rgb", n, h, w, off)
        assert len(op) == 1 and op[0] == dict(cells(n, h, w), name="yuv2rgb", px="u8", form=FORM_NAME[form], count=1), op
        # RGB -> YCbCr: the frames land at the offset the input did NOT have
        x = random_rgb(rng, n, h, w)
        o2 = OFFSETS[(i + 1 + h) % len(OFFSETS)]
        dst, whole = byte_view(n * fb, o2)
        got = e.rgb_to_yuv_dev(torch.from_numpy(x).cuda(), fmt, out=dst.view(n, fb))
        op = e.last_plan()["ops"]
        torch.cuda.synchronize()
        want = np.stack([yuv_ref.rgb_to_yuv(x[i], sub, siting, matrix, range_) for i in range(n)])
        assert got.cpu().numpy().tobytes() == want.tobytes(), ("to yuv", n, h, w, o2)
        assert guards_intact(whole, o2, n * fb), ("to yuv", n, h, w, o2)
        assert len(op) == 1 and op[0] == dict(cells(n, h, w), name="rgb2yuv", px="f32", form=FORM_NAME[form], count=1), op


def test_f32_side_at_every_dword_offset_and_the_host_forms(engines):
    """The f32 image at 4, 8 and 12 bytes into its allocation (the kernels' 16-byte loads are taken where the address allows), a width
    that is a multiple of 4 and one that is not; and the numpy forms of the binding."""
    import torch
    e = engines()
    fmt = fmt_of("420", "left", "bt709", "limited")
    rng = np.random.default_rng(5)
    for h, w in ((6, 64), (5, 67)):
        x = random_rgb(rng, 1, h, w)
        want = yuv_ref.rgb_to_yuv(x[0], "420", "left", "bt709", "limited")
        for off in (0, 4, 8, 12):
            src, _ = byte_view(x.nbytes, off)
            t = src.view(torch.float32).view(1, h, w, 3)
            t.copy_(torch.from_numpy(x))
            got = e.rgb_to_yuv_dev(t, fmt)
            torch.cuda.synchronize()
            assert got.cpu().numpy()[0].tobytes() == want.tobytes(), (h, w, off)
        assert e.rgb_to_yuv(x[0], fmt).tobytes() == want.tobytes()
        assert e.yuv_to_rgb(want, fmt, h, w).tobytes() == yuv_ref.yuv_to_rgb(want, h, w, "420", "left", "bt709", "limited").tobytes()


# ---- 2. the composed call --------------------------------------------------------------------------------------------------------------
def smooth_frames(seed, sub, siting, matrix, range_, n, h, w):
    """Frames of a smooth picture: the restatement's conversion of synth_u8's pixels."""
    px = synth_u8(seed, n, h, w)
    return np.stack([yuv_ref.rgb_to_yuv(px[i].astype(np.float32) / np.float32(255.0), sub, siting, matrix, range_) for i in range(n)])


def chained(e, frames, fmt, h, w, members):
    import torch
    t = torch.from_numpy(frames).cuda()
    rgb = e.yuv_to_rgb_dev(t, fmt, h, w)
    net = e.upscale_f32_dev(rgb) if members == 1 else e.upscale_ensemble_f32_dev(rgb, members=members)
    out = e.rgb_to_yuv_dev(net, fmt)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("members", [1, ALL8], ids=["plain", "ensemble8"])
@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_composed_call_is_its_three_device_calls(engines, precision, factor, members):
    import torch
    e = engines(precision, factor=factor)
    for (sub, siting, matrix, range_, h, w) in (("420", "left", "bt709", "limited", 17, 13), ("444", "center", "bt601", "full", 16, 12)):
        fmt = fmt_of(sub, siting, matrix, range_)
        frames = smooth_frames(factor * 10 + h, sub, siting, matrix, range_, 2, h, w)
        want = chained(e, frames, fmt, h, w, members)
        assert want.shape == (2, yuv_ref.frame_bytes(sub, factor * h, factor * w)) and want[0].tobytes() != want[1].tobytes()
        dev = e.upscale_yuv_dev(torch.from_numpy(frames).cuda(), fmt, h, w, members)
        ops = [o["name"] for o in e.last_plan()["ops"]]
        torch.cuda.synchronize()
        assert dev.cpu().numpy().tobytes() == want.tobytes(), (sub, "dev")
        assert ops[0] == "yuv2rgb" and ops[-1] == "rgb2yuv"
        assert e.upscale_yuv(frames, fmt, h, w, members).tobytes() == want.tobytes(), (sub, "host")
        assert e.upscale_yuv(frames[1], fmt, h, w, members).tobytes() == want[1].tobytes()


def test_composed_call_on_the_bilinear_graph(engines):
    e = engines(graph="bilinear")
    fmt = fmt_of("420", "center", "bt601", "limited")
    frames = smooth_frames(3, "420", "center", "bt601", "limited", 1, 19, 23)
    want = chained(e, frames, fmt, 19, 23, 1)
    assert e.upscale_yuv(frames, fmt, 19, 23).tobytes() == want.tobytes()


ORACLE_CAP = 1e-3     # the share of bytes that may differ from the oracle's, by one level: the project's bar (tests/test_host_cli.py)
ORACLE_GATE = 0.25    # a frame stays only if the f32 oracle against its f64 build differs on less than this share of the cap


def oracle_frames():
    """(name, frame, h, w): a 4:2:0 cut of butterfly_lr.png (48 x 64, MPEG-2 siting, limited BT.709 -- what a clip carries) and one
    seeded noise frame, smoothed as synth_u8 smooths.  A condition on the frames, held on the CPU by tests/test_yuv_cpu.py: the f32
    oracle against its f64 build differs on a share of the output bytes below ORACLE_GATE of the cap (0 of 41472 bytes on either)."""
    px = load_png("butterfly_lr.png")[40:88, 30:94, :3]
    noise = synth_u8(2027, 1, 48, 64)[0]
    return [(name, yuv_ref.rgb_to_yuv(p.astype(np.float32) / np.float32(255.0), "420", "left", "bt709", "limited"), 48, 64)
            for name, p in (("butterfly", px), ("noise", noise))]


def oracle_upscale(params, frame, h, w, f64=False):
    x = yuv_ref.yuv_to_rgb(frame, h, w, "420", "left", "bt709", "limited")
    return yuv_ref.rgb_to_yuv(oracle.forward(params, x[None], f64=f64)[0], "420", "left", "bt709", "limited")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_against_the_oracle(engines, params, precision):
    """yuv_ref -> the oracle's f32 upscale -> yuv_ref against the composed call: the project's own bar for quantised output
    (tests/test_host_cli.py): at most one level, on fewer than 1e-3 of the bytes."""
    e = engines(precision)
    fmt = fmt_of("420", "left", "bt709", "limited")
    for name, frame, h, w in oracle_frames():
        want = oracle_upscale(params["imagenet"], frame, h, w)
        got = e.upscale_yuv(frame, fmt, h, w)
        d = np.abs(got.astype(int) - want.astype(int))
        print(f"{name}, {precision}: max level diff = {d.max()}, share = {(d != 0).mean():.3g}")
        assert got.shape == want.shape and d.max() <= 1 and (d != 0).mean() < ORACLE_CAP


# ---- 3. the frame stream ---------------------------------------------------------------------------------------------------------------
STREAM = ("420", "left", "bt709", "limited", 20, 24)


def stream_frames(count=7):
    sub, siting, matrix, range_, h, w = STREAM
    return smooth_frames(900, sub, siting, matrix, range_, count, h, w)


@pytest.mark.parametrize("slots", [1, 2, 3, 4])
def test_stream_gives_the_synchronous_calls_frames_in_order(engines, slots):
    import rusty_sr_amd as r
    e = engines()
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt_of(sub, siting, matrix, range_)
    frames = stream_frames()
    want = [e.upscale_yuv(f, fmt, h, w) for f in frames]
    assert len({x.tobytes() for x in want}) == len(frames)
    v = r.VideoStream(e, fmt, h, w, slots=slots)
    got = list(v.frames(frames))
    assert v.pending == 0 and len(got) == len(frames)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (slots, i)
    # by hand: fill the ring, and a further acquire is refused without disturbing anything
    from rusty_sr_amd import _lib
    for f in frames[:slots]:
        v.submit(f)
    assert v.pending == slots
    p = C.c_void_p(0)
    assert e._L.sr_video_acquire(v._v, C.byref(p)) == _lib.SR_E_INVALID and not p.value
    with pytest.raises(r.SrError):
        v.submit(frames[0])
    assert v.pending == slots
    for i in range(slots):
        assert v.receive().tobytes() == want[i].tobytes(), (slots, i)
    # nothing pending: receive is refused; submit without acquire too
    assert e._L.sr_video_receive(v._v, C.byref(p)) == _lib.SR_E_INVALID
    assert e._L.sr_video_submit(v._v) == _lib.SR_E_INVALID
    v.close()
    assert e.upscale_yuv(frames[0], fmt, h, w).tobytes() == want[0].tobytes()   # the context still serves


def test_stream_with_an_ensemble_and_at_factor_2(engines):
    import rusty_sr_amd as r
    e = engines("split_f16", factor=2)
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt_of(sub, siting, matrix, range_)
    frames = stream_frames(4)
    want = [e.upscale_yuv(f, fmt, h, w, members=0x03) for f in frames]
    v = r.VideoStream(e, fmt, h, w, slots=2, members=0x03)
    for a, b in zip(v.frames(frames), want):
        assert a.tobytes() == b.tobytes()
    v.close()


def test_destroy_with_frames_in_flight_and_detach(params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt_of(sub, siting, matrix, range_)
    frames = stream_frames(3)
    e = r.Engine(params["imagenet"])
    want = e.upscale_yuv(frames[0], fmt, h, w)
    v = r.VideoStream(e, fmt, h, w, slots=3)
    for f in frames:
        v.submit(f)
    v.close()                                    # frames in flight: waits for them
    assert e.upscale_yuv(frames[0], fmt, h, w).tobytes() == want.tobytes()
    v = r.VideoStream(e, fmt, h, w, slots=2)
    v.submit(frames[0])
    v.submit(frames[1])
    e.close()                                    # the context goes first: the session is drained and detached
    p = C.c_void_p(0)
    L = _lib.lib()
    assert v.pending == -1
    assert L.sr_video_acquire(v._v, C.byref(p)) == _lib.SR_E_INVALID and L.sr_video_receive(v._v, C.byref(p)) == _lib.SR_E_INVALID
    assert L.sr_video_submit(v._v) == _lib.SR_E_INVALID
    v.close()


def test_stream_recomputes_in_f32_when_a_frame_leaves_the_split_domain(params):
    """Parameters with which channel 5 of the first layer leaves the split-half mode's domain on any image (tests/domain_cases.py's
    wiring: nothing reads that channel; its bias is 7e4, the activation case of tests/test_gpu_domain.py), so every frame raises the
    word and the frames still differ: every frame equals the exact-f32 call's, in order, and the context ends in exact f32."""
    import domain_cases
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt_of(sub, siting, matrix, range_)
    frames = stream_frames(5)
    p = domain_cases.wired("f", 5, 1.0)
    domain_cases._view(p, 3, "f_bias")[5] = 7e4
    exact = r.Engine(p, precision="f32")
    want = [exact.upscale_yuv(f, fmt, h, w) for f in frames]
    exact.close()
    assert len({x.tobytes() for x in want}) == len(frames)
    probe = r.Engine(p, precision="split_f16")   # the premise: in the split-half mode a frame of these does leave the domain
    import torch
    probe.upscale_yuv_dev(torch.from_numpy(frames[:1]).cuda(), fmt, h, w)
    torch.cuda.synchronize()
    assert probe._L.sr_check_domain(probe._ctx) == _lib.SR_E_DOMAIN
    probe.close()
    e = r.Engine(p, precision="split_f16")
    v = r.VideoStream(e, fmt, h, w, slots=3)
    got = list(v.frames(frames))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), i
    e.check_domain()                             # the word was cleared
    # the context is in exact f32 now: a device call of a domain-leaving image raises no fault
    import torch
    x = torch.from_numpy(np.random.default_rng(1).random((1, h, w, 3), dtype=np.float32)).cuda()
    e.upscale_f32_dev(x)
    torch.cuda.synchronize()
    assert e._L.sr_check_domain(e._ctx) == _lib.SR_OK
    v.close()
    e.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(engines, params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil = engines(), engines(graph="bilinear")
    down = r.downsample_net()
    h, w, f = 6, 10, 3
    fmt = fmt_of("420", "left", "bt709", "limited")
    fb, ob = yuv_ref.frame_bytes("420", h, w), yuv_ref.frame_bytes("420", f * h, f * w)
    src = torch.from_numpy(smooth_frames(1, "420", "left", "bt709", "limited", 1, h, w)).cuda()
    rgb = torch.zeros((1, f * h, f * w, 3), dtype=torch.float32, device="cuda")
    out, whole = byte_view(f * h * f * w * 12 + 64, 0)
    L, INV = e._L, _lib.SR_E_INVALID
    stream = e._stream_ptr(None, src.device)
    p_in, p_rgb, p_out, pf = C.c_void_p(src.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(fmt)

    def up(ctx=e._ctx, a=p_in, ff=pf, n=1, hh=h, ww=w, b=p_out, members=1):
        return L.sr_upscale_yuv_dev(ctx, a, ff, n, hh, ww, b, members, stream)

    def to_rgb(ctx=e._ctx, a=p_in, ff=pf, n=1, hh=h, ww=w, b=p_out):
        return L.sr_yuv_to_rgb_dev(ctx, a, ff, n, hh, ww, b, stream)

    def to_yuv(ctx=e._ctx, a=p_rgb, ff=pf, n=1, hh=h, ww=w, b=p_out):
        return L.sr_rgb_to_yuv_dev(ctx, a, ff, n, hh, ww, b, stream)

    v = C.c_void_p(0)

    def create(ctx=e._ctx, ff=pf, hh=h, ww=w, slots=3, members=1, o=C.byref(v)):
        return L.sr_video_create(ctx, ff, hh, ww, slots, members, o)

    for call in (up, to_rgb, to_yuv):
        assert call(a=None) == INV and call(b=None) == INV and call(ff=None) == INV
        for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (1, 2 ** 30, w), (1, h, 2 ** 30)):
            assert call(n=n, hh=hh, ww=ww) == INV, (n, hh, ww)
    assert create(ff=None) == INV and create(o=None) == INV
    for hh, ww in ((0, w), (h, 0), (2 ** 30, w)):
        assert create(hh=hh, ww=ww) == INV
    for field in ("subsampling", "siting", "matrix", "range"):
        for bad in (-1, 2, 1 << 20):
            wrong = fmt_of("420", "left", "bt709", "limited")
            setattr(wrong, field, bad)
            assert up(ff=C.byref(wrong)) == INV and to_rgb(ff=C.byref(wrong)) == INV and to_yuv(ff=C.byref(wrong)) == INV
            assert create(ff=C.byref(wrong)) == INV
    for off in (1, 2, 3):                                   # the f32 pointers must be dword-aligned; the frames may start anywhere
        assert to_rgb(b=C.c_void_p(out.data_ptr() + off)) == INV and to_yuv(a=C.c_void_p(rgb.data_ptr() + off)) == INV
    for slots in (0, 9, -1, 1 << 20):
        assert create(slots=slots) == INV
    for members in (0, 256, 1 << 20):
        assert up(members=members) == INV and create(members=members) == INV
    for members in (0, 3, ALL8):                            # members != 1 off sr_net
        assert up(ctx=bil._ctx, members=members) == INV and create(ctx=bil._ctx, members=members) == INV
    assert up(ctx=down._ctx) == INV and create(ctx=down._ctx) == INV      # the downsample graph has no composed call ...
    assert not v.value
    torch.cuda.synchronize()
    assert (whole == 0xA5).all()
    assert to_rgb(ctx=down._ctx) == _lib.SR_OK                             # ... but converts, like any context
    torch.cuda.synchronize()
    want = yuv_ref.yuv_to_rgb(src.cpu().numpy()[0], h, w, "420", "left", "bt709", "limited")
    assert out[:h * w * 12].cpu().numpy().tobytes() == want.tobytes()
    # a live session: null result pointers are refused and disturb nothing
    frame = src.cpu().numpy()[0]
    live = r.VideoStream(e, fmt, h, w, slots=2)
    assert L.sr_video_acquire(live._v, None) == INV and L.sr_video_submit(live._v) == INV      # (nothing was acquired by that)
    live.submit(frame)
    assert L.sr_video_receive(live._v, None) == INV and live.pending == 1
    assert live.receive().tobytes() == e.upscale_yuv(frame, fmt, h, w).tobytes()
    live.close()
    # the host forms, through the binding
    for call in (lambda: e.upscale_yuv(frame, fmt, h, w, members=0), lambda: bil.upscale_yuv(frame, fmt, h, w, members=3),
                 lambda: down.upscale_yuv(frame, fmt, h, w), lambda: r.VideoStream(e, fmt, h, w, slots=0),
                 lambda: r.VideoStream(e, fmt, h, w, slots=9), lambda: r.VideoStream(down, fmt, h, w)):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    with pytest.raises(ValueError):
        e.upscale_yuv(frame[:-1], fmt, h, w)
    down.close()
    # a shape no device can hold is SR_E_NOMEM by arithmetic, and the context still serves
    assert up(hh=150000, ww=150000) == _lib.SR_E_NOMEM
    assert e.upscale_yuv(frame, fmt, h, w).shape == (ob,)


# ---- 5. the CLI ------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rusty_sr_amd", "bin", "rusty_sr")


def split_y4m(data, frame_bytes):
    """(header line, [(FRAME line, payload)]) of a Y4M byte string whose frames are whole."""
    head, rest = data.split(b"\n", 1)
    frames = []
    while rest:
        line, rest = rest.split(b"\n", 1)
        assert len(rest) >= frame_bytes
        frames.append((line, rest[:frame_bytes]))
        rest = rest[frame_bytes:]
    return head, frames


@pytest.mark.parametrize("case", [("420", "left", "limited", 13, 17, "YUV4MPEG2 W17 H13 F25:1 Ip A1:1 C420mpeg2", "YUV4MPEG2 W51 H39 F25:1 Ip A1:1 C420mpeg2"),
                                  ("444", "center", "full", 12, 16, "YUV4MPEG2 W16 H12 F30000:1001 C444 XCOLORRANGE=FULL",
                                   "YUV4MPEG2 W48 H36 F30000:1001 C444 XCOLORRANGE=FULL")], ids=["420mpeg2", "444full"])
def test_cli_video(engines, tmp_path, case):
    import subprocess
    from rusty_sr_amd.build import build_host
    from test_yuv_cpu import y4m_bytes
    build_host()
    sub, siting, range_, h, w, header, want_header = case
    e = engines()
    fmt = fmt_of(sub, siting, "bt601", range_)             # small frames: BT.601 without --matrix
    frames = smooth_frames(40 + h, sub, siting, "bt601", range_, 5, h, w)
    lines = ["FRAME", "FRAME Ip", "FRAME XPTS=2", "FRAME", "FRAME Ip XLAST"]
    stream = y4m_bytes(header, frames, lines)
    fb, ob = yuv_ref.frame_bytes(sub, h, w), yuv_ref.frame_bytes(sub, 3 * h, 3 * w)
    want = [e.upscale_yuv(f, fmt, h, w).tobytes() for f in frames]

    def check(data, count=5):
        head, got = split_y4m(data, ob)
        assert head.decode() == want_header
        assert [g[0].decode() for g in got] == lines[:count]
        for i, g in enumerate(got):
            assert g[1] == want[i], i

    # stdin -> stdout
    res = subprocess.run([CLI, "video", "--timing", "-", "-"], input=stream, capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr
    check(res.stdout)
    assert b"[timing] frames 5, " in res.stderr and b" ms/frame" in res.stderr
    # file -> file, one slot, and --matrix bt709 changes the bytes
    src, out = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(stream)
    res = subprocess.run([CLI, "video", "--slots", "1", str(src), str(out)], capture_output=True, timeout=120)
    assert res.returncode == 0 and res.stdout == b"", res.stderr
    check(out.read_bytes())
    res = subprocess.run([CLI, "video", "--matrix", "bt709", str(src), str(out)], capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr
    fmt709 = fmt_of(sub, siting, "bt709", range_)
    _, got = split_y4m(out.read_bytes(), ob)
    assert got[2][1] == e.upscale_yuv(frames[2], fmt709, h, w).tobytes() and got[2][1] != want[2]
    # a stream cut in the middle of frame 3: exit 1 naming it, frames 0..2 written
    cut = stream[:len(stream) - fb - len(lines[4]) - 1 - fb // 2]
    res = subprocess.run([CLI, "video", "-", "-"], input=cut, capture_output=True, timeout=120)
    assert res.returncode == 1 and b"frame 3 is truncated" in res.stderr, res.stderr
    check(res.stdout, 3)
