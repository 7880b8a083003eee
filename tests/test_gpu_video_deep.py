"""The deep video path on the GPU (include/srhip.h "Deep video"): both conversion kernels against tests/yuv16_ref.py sample for sample and
bit for bit on every grid cell and at every offset of a frame within its 16-byte group, the composed call against its three device calls
chained and against the oracle, the frame stream of sr_video_create16 against the synchronous call, the refusals, and `rusty_sr video
--depth auto`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import yuv16_ref
import yuv_ref
from conftest import load_png, synth_u8
from test_gpu_validation import synthetic_params
from test_gpu_video import byte_view, guards_intact, random_rgb, split_y4m

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
FORM_NAME = {("420", "center"): "420center", ("420", "left"): "420left", ("422", "center"): "422center", ("422", "left"): "422left",
             ("444", "center"): "444"}
# the five forms at depths 10 and 16, one more at 12; the three matrices and both ranges spread over them
CASES = [("420", "center", "bt601", "limited", 10), ("420", "left", "bt709", "limited", 10), ("422", "center", "bt2020", "full", 10),
         ("422", "left", "bt709", "limited", 10), ("444", "center", "bt2020", "limited", 10),
         ("420", "center", "bt2020", "full", 16), ("420", "left", "bt601", "full", 16), ("422", "center", "bt709", "limited", 16),
         ("422", "left", "bt2020", "limited", 16), ("444", "center", "bt601", "full", 16), ("420", "left", "bt2020", "limited", 12)]
SMALL = ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (16, 12), (17, 13))
OFFSETS = (0, 1, 2, 3, 7)      # samples into a 16-byte group
ALL8 = 0xFF


def span():
    from rusty_sr_amd import _lib
    return _lib.SR_YUV_SPAN    # the deep pair cuts rows as the 8-bit pair does


def wide_shapes():
    """Widths either side of a workgroup's SR_YUV_SPAN columns, one by one (the 16-byte groups of a row end at every sample offset), at 3
    rows, and three block columns at 5 rows: the first, an interior and the last block of both grid axes run."""
    s = span()
    return tuple((3, w) for w in range(s - 1, s + 6)) + ((5, 2 * s + 1),)


def fmt_of(sub, siting, matrix, range_, depth):
    from rusty_sr_amd import Yuv16Format
    return Yuv16Format.named(sub, siting, matrix, range_, depth)


def cells(n, h, w):
    return {"n": n, "bx": -(-w // span()), "by": -(-h // 2)}


def dev16(a):
    """A numpy uint16 array on the GPU (an int16 tensor holding the same bits)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).cuda()


def host16(t):
    return t.cpu().numpy().view(np.uint16)


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


def random_frames(rng, sub, n, h, w, depth, range_):
    """Any code of the depth; 0, 2^d - 1, 65535 (outside the depth's own codes below 16 bits) and codes below the range's limits among them."""
    f = rng.integers(0, 1 << depth, (n, yuv16_ref.frame_samples(sub, h, w)), dtype=np.uint16)
    flat = f.reshape(-1)
    flat[::7] = 0
    flat[3::11] = (1 << depth) - 1
    flat[5::13] = 65535
    flat[2::17] = 3 if range_ == "limited" else 1
    return f


def random_rgb16(rng, n, h, w, depth):
    """random_rgb of the 8-bit tests (f32 in [-2, 3]; +-1e30, the infinities, NaN; grey 0.5) with the grey whose luma sits on a rounding
    tie at this depth as well: 2^-(d - 7) in limited range (219 s v = 109.5), 0.5 in full range ((2^d - 1) / 2)."""
    x = random_rgb(rng, n, h, w)
    flat = x.reshape(-1, 3)
    flat[rng.integers(0, len(flat), max(1, len(flat) // 9))] = np.float32(2.0 ** -(depth - 7))
    return x


# ---- 1. the two launches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_conversions_are_the_restatement(engines, case):
    """Every small shape with the frames at every sample offset 0, 1, 2, 3, 7 of a 16-byte group at n = 1 and at one more at n = 2 (in
    and out rotate against each other), the wide shapes at n = 2: the f32 RGB equals yuv16_ref bit for bit, the frames sample for
    sample, the bytes around the outputs stay, and the recorded op names the grid the shape gives."""
    import torch
    e = engines()
    sub, siting, matrix, range_, depth = case
    fmt = fmt_of(*case)
    rng = np.random.default_rng(sum(map(ord, sub + siting + matrix + range_)) + depth)
    runs = [(1, h, w, off) for (h, w) in SMALL for off in OFFSETS] + [(2, h, w, OFFSETS[(h + w) % 5]) for (h, w) in SMALL]
    runs += [(2, h, w, OFFSETS[(w + h) % 5]) for (h, w) in wide_shapes()]
    for n, h, w, off in runs:
        fs = yuv16_ref.frame_samples(sub, h, w)
        # YCbCr -> RGB
        frames = random_frames(rng, sub, n, h, w, depth, range_)
        src, _ = byte_view(2 * n * fs, 2 * off)
        src.copy_(torch.from_numpy(frames.reshape(-1).view(np.uint8)))
        f_off = 4 * (off % 4)
        dst, whole = byte_view(n * h * w * 12, f_off)
        out = dst.view(torch.float32).view(n, h, w, 3)
        assert e.yuv16_to_rgb_dev(src.view(torch.int16).view(n, fs), fmt, h, w, out=out) is out
        op = e.last_plan()["ops"]
        torch.cuda.synchronize()
        want = np.stack([yuv16_ref.yuv_to_rgb(frames[i], h, w, *case) for i in range(n)])
        assert out.cpu().numpy().tobytes() == want.tobytes(), ("to rgb", n, h, w, off)
        assert guards_intact(whole, f_off, n * h * w * 12), ("to rgb", n, h, w, off)
        assert len(op) == 1 and op[0] == dict(cells(n, h, w), name="yuv16_to_rgb", px="f32", form=FORM_NAME[(sub, siting)], count=1), op
        # RGB -> YCbCr: the frames land at an offset the input did NOT have
        x = random_rgb16(rng, n, h, w, depth)
        o2 = OFFSETS[(OFFSETS.index(off) + 1 + h) % 5]
        dst, whole = byte_view(2 * n * fs, 2 * o2)
        got = e.rgb_to_yuv16_dev(torch.from_numpy(x).cuda(), fmt, out=dst.view(torch.int16).view(n, fs))
        op = e.last_plan()["ops"]
        torch.cuda.synchronize()
        want = np.stack([yuv16_ref.rgb_to_yuv(x[i], *case) for i in range(n)])
        assert host16(got).tobytes() == want.tobytes(), ("to yuv", n, h, w, o2)
        assert guards_intact(whole, 2 * o2, 2 * n * fs), ("to yuv", n, h, w, o2)
        assert len(op) == 1 and op[0] == dict(cells(n, h, w), name="rgb_to_yuv16", px="f32", form=FORM_NAME[(sub, siting)], count=1), op


def test_f32_side_at_every_dword_offset_and_the_host_forms(engines):
    """The f32 image at 0, 4, 8 and 12 bytes into its allocation, read and written (the kernels' 16-byte loads and stores are taken where
    the address allows), a width that is a multiple of 4 and one that is not; and the numpy forms of the binding."""
    import torch
    e = engines()
    case = ("422", "left", "bt2020", "limited", 10)
    fmt = fmt_of(*case)
    rng = np.random.default_rng(5)
    for h, w in ((6, 64), (5, 67)):
        x = random_rgb16(rng, 1, h, w, 10)
        want = yuv16_ref.rgb_to_yuv(x[0], *case)
        rgb = yuv16_ref.yuv_to_rgb(want, h, w, *case)
        for off in (0, 4, 8, 12):
            src, _ = byte_view(x.nbytes, off)
            t = src.view(torch.float32).view(1, h, w, 3)
            t.copy_(torch.from_numpy(x))
            got = e.rgb_to_yuv16_dev(t, fmt)
            dst, whole = byte_view(x.nbytes, off)
            back = e.yuv16_to_rgb_dev(got, fmt, h, w, out=dst.view(torch.float32).view(1, h, w, 3))
            torch.cuda.synchronize()
            assert host16(got)[0].tobytes() == want.tobytes(), (h, w, off)
            assert back.cpu().numpy()[0].tobytes() == rgb.tobytes() and guards_intact(whole, off, x.nbytes), (h, w, off)
        assert e.rgb_to_yuv16(x[0], fmt).tobytes() == want.tobytes()
        assert e.yuv16_to_rgb(want, fmt, h, w).tobytes() == rgb.tobytes()


# ---- 2. the composed call --------------------------------------------------------------------------------------------------------------
def smooth_frames(seed, case, n, h, w):
    """Frames of a smooth picture: the restatement's conversion of synth_u8's pixels."""
    px = synth_u8(seed, n, h, w)
    return np.stack([yuv16_ref.rgb_to_yuv(px[i].astype(np.float32) / np.float32(255.0), *case) for i in range(n)])


def chained(e, frames, fmt, h, w, members):
    import torch
    rgb = e.yuv16_to_rgb_dev(dev16(frames), fmt, h, w)
    net = e.upscale_f32_dev(rgb) if members == 1 else e.upscale_ensemble_f32_dev(rgb, members=members)
    out = e.rgb_to_yuv16_dev(net, fmt)
    torch.cuda.synchronize()
    return host16(out)


COMPOSED = (("420", "left", "bt709", "limited", 10, 17, 13), ("422", "center", "bt2020", "full", 12, 16, 12))


@pytest.mark.parametrize("members", [1, ALL8], ids=["plain", "ensemble8"])
@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_composed_call_is_its_three_device_calls(engines, precision, factor, members):
    import torch
    e = engines(precision, factor=factor)
    for *case, h, w in COMPOSED:
        fmt = fmt_of(*case)
        frames = smooth_frames(factor * 10 + h, case, 2, h, w)
        want = chained(e, frames, fmt, h, w, members)
        assert want.shape == (2, yuv16_ref.frame_samples(case[0], factor * h, factor * w)) and want[0].tobytes() != want[1].tobytes()
        dev = e.upscale_yuv16_dev(dev16(frames), fmt, h, w, members)
        ops = [o["name"] for o in e.last_plan()["ops"]]
        torch.cuda.synchronize()
        assert host16(dev).tobytes() == want.tobytes(), (case, "dev")
        assert ops[0] == "yuv16_to_rgb" and ops[-1] == "rgb_to_yuv16"
        assert e.upscale_yuv16(frames, fmt, h, w, members).tobytes() == want.tobytes(), (case, "host")
        assert e.upscale_yuv16(frames[1], fmt, h, w, members).tobytes() == want[1].tobytes()


def test_composed_call_on_the_bilinear_graph(engines):
    e = engines(graph="bilinear")
    case = ("444", "center", "bt601", "limited", 16)
    frames = smooth_frames(3, case, 1, 19, 23)
    want = chained(e, frames, fmt_of(*case), 19, 23, 1)
    assert e.upscale_yuv16(frames, fmt_of(*case), 19, 23).tobytes() == want.tobytes()


ORACLE_CASES = [("limited", 10), ("limited", 12), ("limited", 16), ("full", 16)]


def level_bound(k):
    """Levels a sample may differ from the oracle route's: the project's f32 parity bar, 1e-4 of the unit range, is 1e-4 span levels --
    span = ky for luma, kc for chroma: the chroma gain is bounded by kc because ir 2 (1 - Kr) = 1 -- and one more for the rounding
    itself: 1 level at 10 and 12 bits, 6 (limited) and 7 (full) at 16."""
    return int(np.floor(1e-4 * float(k.ky))) + 1, int(np.floor(1e-4 * float(k.kc))) + 1


@pytest.mark.parametrize("range_,depth", ORACLE_CASES)
def test_against_the_oracle(engines, params, range_, depth):
    """yuv16_ref -> the oracle's f32 upscale -> yuv16_ref against the composed call in exact f32, on a 4:2:0 cut of butterfly_lr.png
    promoted to the depth and on a seeded noise frame: every sample within floor(1e-4 span) + 1 levels.
    Observed on an MI355X: see DESIGN.md 4u."""
    e = engines("f32")
    case = ("420", "left", "bt709", range_, depth)
    k = yuv16_ref.Rule("bt709", range_, depth)
    by, bc = level_bound(k)
    assert (by, bc) == {10: (1, 1), 12: (1, 1), 16: (6, 6) if range_ == "limited" else (7, 7)}[depth]
    h, w = 48, 64
    for name, px in (("butterfly", load_png("butterfly_lr.png")[40:88, 30:94, :3]), ("noise", synth_u8(2027, 1, h, w)[0])):
        frame = yuv16_ref.rgb_to_yuv(px.astype(np.float32) / np.float32(255.0), *case)
        x = yuv16_ref.yuv_to_rgb(frame, h, w, *case)
        want = yuv16_ref.rgb_to_yuv(oracle.forward(params["imagenet"], x[None])[0], *case)
        got = e.upscale_yuv16(frame, fmt_of(*case), h, w)
        assert got.shape == want.shape
        d = np.abs(got.astype(int) - want.astype(int))
        dy, dc = d[:9 * h * w], d[9 * h * w:]
        print(f"{name}, depth {depth} {range_}: max level diff luma {dy.max()} (bound {by}), chroma {dc.max()} (bound {bc}), "
              f"share differing {(d != 0).mean():.3g}")
        assert dy.max() <= by and dc.max() <= bc, name


# ---- 3. the frame stream ---------------------------------------------------------------------------------------------------------------
STREAM = ("420", "left", "bt709", "limited", 10)
STREAM_HW = (20, 24)


@pytest.mark.parametrize("slots", [1, 3])
def test_stream_gives_the_synchronous_calls_frames_in_order(engines, slots):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e = engines()
    h, w = STREAM_HW
    fmt = fmt_of(*STREAM)
    frames = smooth_frames(900, STREAM, 7, h, w)
    want = [e.upscale_yuv16(f, fmt, h, w) for f in frames]
    assert len({x.tobytes() for x in want}) == len(frames)
    v = r.VideoStream(e, fmt, h, w, slots=slots)
    assert v.in_bytes == yuv16_ref.frame_bytes("420", h, w) and v.out_bytes == yuv16_ref.frame_bytes("420", 3 * h, 3 * w)
    got = list(v.frames(frames))
    assert v.pending == 0 and len(got) == len(frames)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (slots, i)
    for f in frames[:slots]:                                  # a full ring refuses a further acquire without disturbing anything
        v.submit(f)
    p = C.c_void_p(0)
    assert e._L.sr_video_acquire(v._v, C.byref(p)) == _lib.SR_E_INVALID and v.pending == slots
    for i in range(slots):
        assert v.receive().tobytes() == want[i].tobytes(), (slots, i)
    v.close()
    assert e.upscale_yuv16(frames[0], fmt, h, w).tobytes() == want[0].tobytes()   # the context still serves


def test_destroy_with_frames_in_flight(params):
    import rusty_sr_amd as r
    h, w = STREAM_HW
    fmt = fmt_of(*STREAM)
    frames = smooth_frames(900, STREAM, 3, h, w)
    e = r.Engine(params["imagenet"])
    want = e.upscale_yuv16(frames[0], fmt, h, w)
    v = r.VideoStream(e, fmt, h, w, slots=3)
    for f in frames:
        v.submit(f)
    v.close()                                    # frames in flight: waits for them
    assert e.upscale_yuv16(frames[0], fmt, h, w).tobytes() == want.tobytes()
    v = r.VideoStream(e, fmt, h, w, slots=2)
    v.submit(frames[0])
    e.close()                                    # the context goes first: the session is drained and detached
    assert v.pending == -1
    v.close()


def test_stream_recomputes_in_f32_when_a_frame_leaves_the_split_domain():
    """tests/test_gpu_video.py's method with a deep format: parameters with which every frame leaves the split-half mode's domain, so
    every frame equals the exact-f32 call's, in order, and the context ends in exact f32."""
    import domain_cases
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    h, w = STREAM_HW
    fmt = fmt_of(*STREAM)
    frames = smooth_frames(900, STREAM, 5, h, w)
    p = domain_cases.wired("f", 5, 1.0)
    domain_cases._view(p, 3, "f_bias")[5] = 7e4
    exact = r.Engine(p, precision="f32")
    want = [exact.upscale_yuv16(f, fmt, h, w) for f in frames]
    exact.close()
    assert len({x.tobytes() for x in want}) == len(frames)
    import torch
    probe = r.Engine(p, precision="split_f16")   # the premise: in the split-half mode a frame of these does leave the domain
    probe.upscale_yuv16_dev(dev16(frames[:1]), fmt, h, w)
    torch.cuda.synchronize()
    assert probe._L.sr_check_domain(probe._ctx) == _lib.SR_E_DOMAIN
    probe.close()
    e = r.Engine(p, precision="split_f16")
    v = r.VideoStream(e, fmt, h, w, slots=3)
    got = list(v.frames(frames))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.view(np.uint8).tobytes(), i
    e.check_domain()                             # the word was cleared
    assert e.upscale_yuv16(frames[0], fmt, h, w).tobytes() == want[0].tobytes()   # the context is in exact f32 now
    assert e._L.sr_check_domain(e._ctx) == _lib.SR_OK
    v.close()
    e.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(engines):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil = engines(), engines(graph="bilinear")
    down = r.downsample_net()
    h, w, f = 6, 10, 3
    case = ("422", "left", "bt2020", "limited", 10)
    fmt = fmt_of(*case)
    src = dev16(smooth_frames(1, case, 1, h, w))
    rgb = torch.zeros((1, f * h, f * w, 3), dtype=torch.float32, device="cuda")
    out, whole = byte_view(f * h * f * w * 12 + 64, 0)
    L, INV = e._L, _lib.SR_E_INVALID
    stream = e._stream_ptr(None, src.device)
    p_in, p_rgb, p_out, pf = C.c_void_p(src.data_ptr()), C.c_void_p(rgb.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(fmt)

    def up(ctx=e._ctx, a=p_in, ff=pf, n=1, hh=h, ww=w, b=p_out, members=1):
        return L.sr_upscale_yuv16_dev(ctx, a, ff, n, hh, ww, b, members, stream)

    def to_rgb(ctx=e._ctx, a=p_in, ff=pf, n=1, hh=h, ww=w, b=p_out):
        return L.sr_yuv16_to_rgb_dev(ctx, a, ff, n, hh, ww, b, stream)

    def to_yuv(ctx=e._ctx, a=p_rgb, ff=pf, n=1, hh=h, ww=w, b=p_out):
        return L.sr_rgb_to_yuv16_dev(ctx, a, ff, n, hh, ww, b, stream)

    v = C.c_void_p(0)

    def create(ctx=e._ctx, ff=pf, hh=h, ww=w, slots=3, members=1, o=C.byref(v)):
        return L.sr_video_create16(ctx, ff, hh, ww, slots, members, o)

    for call in (up, to_rgb, to_yuv):
        assert call(a=None) == INV and call(b=None) == INV and call(ff=None) == INV
        for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (1, 2 ** 30, w), (1, h, 2 ** 30)):
            assert call(n=n, hh=hh, ww=ww) == INV, (n, hh, ww)
    assert create(ff=None) == INV and create(o=None) == INV
    for hh, ww in ((0, w), (h, 0), (2 ** 30, w)):
        assert create(hh=hh, ww=ww) == INV
    for field, bads in (("subsampling", (-1, 3, 1 << 20)), ("siting", (-1, 2, 1 << 20)), ("matrix", (-1, 3, 1 << 20)), ("range", (-1, 2, 1 << 20)),
                        ("depth", (-1, 0, 8, 17, 1 << 20))):
        for bad in bads:
            wrong = fmt_of(*case)
            setattr(wrong, field, bad)
            assert up(ff=C.byref(wrong)) == INV and to_rgb(ff=C.byref(wrong)) == INV and to_yuv(ff=C.byref(wrong)) == INV, (field, bad)
            assert create(ff=C.byref(wrong)) == INV, (field, bad)
    for off in (1, 2, 3):                                   # the f32 pointers must be dword-aligned ...
        assert to_rgb(b=C.c_void_p(out.data_ptr() + off)) == INV and to_yuv(a=C.c_void_p(rgb.data_ptr() + off)) == INV
    odd_in, odd_out = C.c_void_p(src.data_ptr() + 1), C.c_void_p(out.data_ptr() + 1)     # ... and the frames 2-byte aligned
    assert to_rgb(a=odd_in) == INV and to_yuv(b=odd_out) == INV and up(a=odd_in) == INV and up(b=odd_out) == INV
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
    want = yuv16_ref.yuv_to_rgb(host16(src)[0], h, w, *case)
    assert out[:h * w * 12].cpu().numpy().tobytes() == want.tobytes()
    frame = host16(src)[0]
    for call in (lambda: e.upscale_yuv16(frame, fmt, h, w, members=0), lambda: bil.upscale_yuv16(frame, fmt, h, w, members=3),
                 lambda: down.upscale_yuv16(frame, fmt, h, w), lambda: r.VideoStream(e, fmt, h, w, slots=0),
                 lambda: r.VideoStream(down, fmt, h, w)):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    with pytest.raises(ValueError):
        e.upscale_yuv16(frame[:-1], fmt, h, w)
    down.close()
    # a shape no device can hold is SR_E_NOMEM by arithmetic, and the context still serves
    assert up(hh=150000, ww=150000) == _lib.SR_E_NOMEM
    assert e.upscale_yuv16(frame, fmt, h, w).shape == (yuv16_ref.frame_samples("422", f * h, f * w),)


# ---- 5. the CLI ------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rusty_sr_amd", "bin", "rusty_sr")


@pytest.mark.parametrize("tag,sub", [("C420p10", "420"), ("C422p10", "422")])
def test_cli_video_depth_auto(engines, tag, sub):
    """A deep stream through pipes against the library call: the tags repeated with W and H x 3, the FRAME lines passed through, chroma
    read as co-sited, BT.601 at this size; --matrix bt2020 and --siting center change the bytes as the library says."""
    from rusty_sr_amd.build import build_host
    from test_yuv_cpu import y4m_bytes
    build_host()
    e = engines()
    h, w = 13, 17
    case = (sub, "left", "bt601", "limited", 10)
    frames = smooth_frames(40 + h, case, 4, h, w)
    lines = ["FRAME", "FRAME Ip", "FRAME XPTS=2", "FRAME"]
    stream = y4m_bytes(f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 {tag}", [f.tobytes() for f in frames], lines)
    ob = yuv16_ref.frame_bytes(sub, 3 * h, 3 * w)
    for args, c in (((), case), (("--matrix", "bt2020", "--siting", "center", "--slots", "1"), (sub, "center", "bt2020", "limited", 10))):
        want = [e.upscale_yuv16(f, fmt_of(*c), h, w).tobytes() for f in frames]
        res = subprocess.run([CLI, "video", "--depth", "auto", *args, "-", "-"], input=stream, capture_output=True, timeout=120)
        assert res.returncode == 0, res.stderr
        head, got = split_y4m(res.stdout, ob)
        assert head.decode() == f"YUV4MPEG2 W{3 * w} H{3 * h} F25:1 Ip A1:1 {tag}"
        assert [g[0].decode() for g in got] == lines
        for i, g in enumerate(got):
            assert g[1] == want[i], (args, i)


def test_cli_depth_auto_on_an_8_bit_stream_is_the_plain_invocation():
    from rusty_sr_amd.build import build_host
    from test_yuv_cpu import y4m_bytes
    build_host()
    h, w = 13, 17
    px = synth_u8(53, 3, h, w)
    frames = [yuv_ref.rgb_to_yuv(p.astype(np.float32) / np.float32(255.0), "420", "left", "bt601", "limited") for p in px]
    stream = y4m_bytes(f"YUV4MPEG2 W{w} H{h} F25:1 C420mpeg2", frames)
    plain = subprocess.run([CLI, "video", "-", "-"], input=stream, capture_output=True, timeout=120)
    auto = subprocess.run([CLI, "video", "--depth", "auto", "-", "-"], input=stream, capture_output=True, timeout=120)
    eight = subprocess.run([CLI, "video", "--depth", "8", "-", "-"], input=stream, capture_output=True, timeout=120)
    assert plain.returncode == 0 and auto.returncode == 0 and eight.returncode == 0, (plain.stderr, auto.stderr)
    assert len(plain.stdout) > 3 * yuv_ref.frame_bytes("420", 3 * h, 3 * w)
    assert auto.stdout == plain.stdout and eight.stdout == plain.stdout and auto.stderr == plain.stderr
