"""Video at any size on the GPU (include/srhip.h "Video at any size").  Every comparison is on bytes, and every reference
is the chain of existing device calls the new paths are defined by:
  1. the operator, Engine.resize_to_yuv[16], against Engine.resize (f32 -> f32) followed by Engine.rgb_to_yuv[16], on shapes chosen for
     the kernel's edges, every filter, both resize spaces, values outside [0, 1], infinities and NaN, on two contexts and with either
     number of row pairs a workgroup takes;
  2. the composed call against yuv_to_rgb_dev -> upscale_f32_dev (or the ensemble) -> resize_dev -> rgb_to_yuv_dev;
  3. the frame stream against the synchronous call, frame by frame, a frame that leaves the split-half domain among them;
  4. the refusals, with the output untouched and the context / session usable afterwards;
  5. the command line end to end on generated Y4M streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import yuv16_ref
import yuv_ref
from test_gpu_video import byte_view, random_rgb, smooth_frames as smooth_frames8, split_y4m
from test_gpu_video_deep import dev16, host16, smooth_frames as smooth_frames16
from test_gpu_validation import synthetic_params

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
# 8-bit: 4:2:0 under either siting and 4:4:4; deep: the five forms at depths 10 and 16; both ranges, BT.601 / 709 and (deep) BT.2020
CASES8 = [("420", "center", "bt601", "limited"), ("420", "left", "bt709", "full"), ("444", "center", "bt709", "limited")]
CASES16 = [("420", "center", "bt601", "limited", 10), ("420", "left", "bt709", "limited", 10), ("422", "center", "bt2020", "full", 10),
           ("422", "left", "bt709", "limited", 10), ("444", "center", "bt2020", "limited", 10),
           ("420", "center", "bt2020", "full", 16), ("420", "left", "bt601", "full", 16), ("422", "center", "bt709", "limited", 16),
           ("422", "left", "bt2020", "limited", 16), ("444", "center", "bt601", "full", 16)]
# ((h, w), (oh, ow), filter, srgb_space): h, w are the network's f32 output, oh, ow the final frame
SHAPES = [
    ((5, 700), (3, 2051), "lanczos3", False),   # three workgroups across, a ragged last thread (2051 = 2 x 1024 + 3); the left column twice
    ((9, 40), (5, 27), "lanczos3", False),      # odd oh and ow
    ((1, 1), (1, 1), "lanczos3", False),        # one-sample axes
    ((7, 9), (1, 1), "lanczos3", False),
    ((1, 13), (6, 13), "lanczos3", False),      # one input row
    ((60, 8), (12, 6), "lanczos3", False),      # a vertical shrink of 5: 30 taps, clipped at both borders
    ((4, 8), (11, 16), "lanczos3", False),      # a vertical enlargement
    ((12, 12), (4, 4), "box", False),           # a shrinking box, whose windows abut
    ((6, 10), (7, 13), "lanczos3", False),      # ow % 4 = 1, 2, 3: rows of the intermediate off the 16-byte grid
    ((6, 10), (7, 14), "lanczos3", False),
    ((6, 10), (7, 15), "lanczos3", False),
    ((9, 40), (5, 27), "box", False),           # every filter, both spaces
    ((9, 40), (5, 27), "triangle", True),
    ((9, 40), (5, 27), "catrom", False),
    ((9, 40), (5, 27), "lanczos3", True),
    ((4, 8), (11, 16), "catrom", True),
    ((5, 700), (3, 2051), "triangle", True),
]
N = 2   # with odd sizes the second frame's planes start at odd byte offsets


def fmt8(case):
    from rusty_sr_amd import YuvFormat
    return YuvFormat.named(*case)


def fmt16(case):
    from rusty_sr_amd import Yuv16Format
    return Yuv16Format.named(*case)


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    made = {}

    def get(precision="f32", factor=3, graph="sr_net", which=0):
        k = (precision, factor, graph, which)
        if k not in made:
            if graph != "sr_net":
                made[k] = r.Engine(graph=graph)
            else:
                p = params["imagenet"] if factor == 3 else synthetic_params(factor, 100 + factor)
                made[k] = r.Engine(p, device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def resized(engines):
    """The inputs of SHAPES and their f32 resampling by the existing call -- computed once, shared by every format; no test writes to them."""
    e = engines()
    out = []
    for i, ((h, w), size, flt, srgb) in enumerate(SHAPES):
        x = random_rgb(np.random.default_rng(500 + i), N, h, w)
        x[0, 0, 0, 0] = np.float32(-0.75)            # (whatever the draws gave: a negative, a value above 1, an infinity and a NaN)
        if x[0].size >= 12:
            x.reshape(-1)[[1, 5, 9]] = np.array([2.5, np.inf, np.nan], np.float32)
        mid = e.resize(x, size, flt, srgb)
        assert mid.shape == (N,) + size + (3,) and mid.dtype == np.float32
        out.append((x, mid))
    return out


def _operator_case(engines, resized, to_yuv, resize_to_yuv, form, deep):
    """to_yuv(e, mid) is the chain's last link, resize_to_yuv(e, x, size, flt, srgb) the call under test.  It runs four ways, all held to
    the same bytes: the fused kernel with two row pairs a workgroup and with one, the chain inside the library, and the library's own
    rule for the format class, which is one of those."""
    from rusty_sr_amd import _lib
    e, other = engines(), engines(which=1)
    to_name = "rgb_to_yuv16" if deep else "rgb2yuv"
    try:
        for ((h, w), (oh, ow), flt, srgb), (x, mid) in zip(SHAPES, resized):
            want = to_yuv(e, mid)
            bx = -(-ow // _lib.SR_YUV_SPAN)
            e.set_experiment("vyuv", "2")
            got = resize_to_yuv(e, x, (oh, ow), flt, srgb)
            ops = e.last_plan()["ops"]
            assert got.dtype == want.dtype and got.shape == want.shape
            assert got.tobytes() == want.tobytes(), ("two pairs", (h, w), (oh, ow), flt, srgb)
            assert [o["name"] for o in ops] == ["resize_h", "resize_v_yuv"], ops
            assert ops[1]["n"] == N and ops[1]["bx"] == bx and ops[1]["by"] == -(-oh // 4) and ops[1]["form"] == form, ops
            other.set_experiment("vyuv", "1")        # a second context
            again = resize_to_yuv(other, x, (oh, ow), flt, srgb)
            assert other.last_plan()["ops"][1]["by"] == -(-oh // 2)
            assert again.tobytes() == want.tobytes(), ("one pair, second context", (h, w), (oh, ow), flt, srgb)
            other.set_experiment("vyuv", "chain")
            again = resize_to_yuv(other, x, (oh, ow), flt, srgb)
            ops = other.last_plan()["ops"]
            assert [o["name"] for o in ops] == ["resize_h", "resize_v", to_name], ops
            assert ops[2]["bx"] == bx and ops[2]["by"] == -(-oh // 2) and ops[2]["form"] == form, ops
            assert again.tobytes() == want.tobytes(), ("chain", (h, w), (oh, ow), flt, srgb)
            e.set_experiment("vyuv", "")             # the rule: either of the two, the same bytes
            got = resize_to_yuv(e, x, (oh, ow), flt, srgb)
            assert [o["name"] for o in e.last_plan()["ops"]] in (["resize_h", "resize_v_yuv"], ["resize_h", "resize_v", to_name])
            assert got.tobytes() == want.tobytes(), ("rule", (h, w), (oh, ow), flt, srgb)
            assert resize_to_yuv(e, x[1], (oh, ow), flt, srgb).tobytes() == want[1].tobytes()   # one image, not a batch
    finally:
        e.set_experiment("vyuv", "")
        other.set_experiment("vyuv", "")


def test_vyuv_takes_its_four_values_alone(engines):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e = engines()
    for bad in ("0", "3", "fused", "Chain", " 1"):
        with pytest.raises(r.SrError) as err:
            e.set_experiment("vyuv", bad)
        assert err.value.status == _lib.SR_E_INVALID
    for good in ("1", "2", "chain", ""):
        e.set_experiment("vyuv", good)


FORM = {("420", "center"): "420center", ("420", "left"): "420left", ("422", "center"): "422center", ("422", "left"): "422left",
        ("444", "center"): "444"}


# ---- 1. the operator against the chain ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES8, ids=lambda c: "-".join(map(str, c)))
def test_operator_is_the_chain(engines, resized, case):
    fmt = fmt8(case)
    _operator_case(engines, resized, lambda e, mid: e.rgb_to_yuv(mid, fmt),
                   lambda e, x, size, flt, srgb: e.resize_to_yuv(x, fmt, size, flt, srgb), FORM[case[:2]], False)


@pytest.mark.parametrize("case", CASES16, ids=lambda c: "-".join(map(str, c)))
def test_operator_is_the_chain_deep(engines, resized, case):
    fmt = fmt16(case)
    _operator_case(engines, resized, lambda e, mid: e.rgb_to_yuv16(mid, fmt),
                   lambda e, x, size, flt, srgb: e.resize_to_yuv16(x, fmt, size, flt, srgb), FORM[case[:2]], True)


def test_operator_on_any_graph_and_into_the_callers_array(engines, resized):
    """The operator needs no network: a bilinear context runs it; `out` is filled in place."""
    (h, w), size, flt, srgb = SHAPES[1]
    x, mid = resized[1]
    fmt = fmt8(CASES8[1])
    bil = engines(graph="bilinear")
    want = engines().rgb_to_yuv(mid, fmt)
    out = np.zeros(want.shape, np.uint8)
    assert bil.resize_to_yuv(x, fmt, size, flt, srgb, out=out).tobytes() == want.tobytes() and out.tobytes() == want.tobytes()


# ---- 2. the composed call ----------------------------------------------------------------------------------------------------------
def chained_sized(e, frames, fmt, h, w, size, flt, srgb, members, deep):
    import torch
    rgb = e.yuv16_to_rgb_dev(dev16(frames), fmt, h, w) if deep else e.yuv_to_rgb_dev(torch.from_numpy(frames).cuda(), fmt, h, w)
    net = e.upscale_f32_dev(rgb) if members == 1 else e.upscale_ensemble_f32_dev(rgb, members=members)
    res = e.resize_dev(net, size, "f32", flt, srgb)
    out = e.rgb_to_yuv16_dev(res, fmt) if deep else e.rgb_to_yuv_dev(res, fmt)
    torch.cuda.synchronize()
    return host16(out) if deep else out.cpu().numpy()


def sizes_around(f, h, w):
    """A size below, the size of, and a size above the network's own output."""
    return ((f * h - 5, f * w - 7), (f * h, f * w), (f * h + 7, f * w + 5))


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_composed_call_is_the_chain(engines, precision, factor):
    e = engines(precision, factor=factor)
    case8, case16 = ("420", "left", "bt709", "limited"), ("422", "center", "bt2020", "full", 10)
    runs = [(False, case8, fmt8(case8), smooth_frames8(factor * 10 + 1, *case8, 2, 18, 24), 18, 24),
            (True, case16, fmt16(case16), smooth_frames16(factor * 10 + 2, case16, 2, 13, 10), 13, 10)]
    for deep, case, fmt, frames, h, w in runs:
        call = e.upscale_yuv16_sized if deep else e.upscale_yuv_sized
        for k, size in enumerate(sizes_around(factor, h, w)):
            flt, srgb = ("lanczos3", False) if k != 2 else ("catrom", True)
            members = 0x21 if k == 0 else 1                                   # one ensemble mask: the identity and a rotation
            want = chained_sized(e, frames, fmt, h, w, size, flt, srgb, members, deep)
            assert want[0].tobytes() != want[1].tobytes()
            got = call(frames, fmt, h, w, size, flt, srgb, members)
            ops = [o["name"] for o in e.last_plan()["ops"]]
            assert got.tobytes() == want.tobytes(), (deep, size, members)
            assert ops[0] == ("yuv16_to_rgb" if deep else "yuv2rgb"), ops
            assert ops[-2:] == ["resize_h", "resize_v_yuv"] or ops[-3:] == ["resize_h", "resize_v", "rgb_to_yuv16" if deep else "rgb2yuv"], ops
            for mode in ("2", "chain"):                                       # ... and both ways by force
                e.set_experiment("vyuv", mode)
                try:
                    assert call(frames, fmt, h, w, size, flt, srgb, members).tobytes() == want.tobytes(), (deep, size, members, mode)
                finally:
                    e.set_experiment("vyuv", "")
            assert call(frames[1], fmt, h, w, size, flt, srgb, members).tobytes() == want[1].tobytes()
    # what the plain call gives is still the plain chain's
    deep, case, fmt, frames, h, w = runs[0]
    import torch
    plain = e.rgb_to_yuv_dev(e.upscale_f32_dev(e.yuv_to_rgb_dev(torch.from_numpy(frames).cuda(), fmt, h, w)), fmt)
    torch.cuda.synchronize()
    assert e.upscale_yuv(frames, fmt, h, w).tobytes() == plain.cpu().numpy().tobytes()


def test_composed_call_on_the_bilinear_graph_and_its_timing(engines):
    e = engines(graph="bilinear")
    case = ("420", "center", "bt601", "limited")
    fmt = fmt8(case)
    frames = smooth_frames8(3, *case, 1, 18, 24)
    for size in sizes_around(3, 18, 24):
        want = chained_sized(e, frames, fmt, 18, 24, size, "lanczos3", False, 1, False)
        assert e.upscale_yuv_sized(frames, fmt, 18, 24, size).tobytes() == want.tobytes()
    e.set_profiling(True)
    try:
        e.upscale_yuv_sized(frames, fmt, 18, 24, (40, 50))
        t = e.last_timing()
        assert t["total_ms"] > 0 and t["h2d_ms"] > 0 and t["d2h_ms"] > 0, t
    finally:
        e.set_profiling(False)


# ---- 3. the frame stream -----------------------------------------------------------------------------------------------------------
STREAM = ("420", "left", "bt709", "limited", 20, 24)
STREAM_SIZE = (45, 50)


@pytest.mark.parametrize("slots", [1, 2, 3])
def test_stream_gives_the_synchronous_calls_frames_in_order(engines, slots):
    import rusty_sr_amd as r
    e = engines()
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt8(STREAM[:4])
    frames = smooth_frames8(900, sub, siting, matrix, range_, 5, h, w)
    want = [e.upscale_yuv_sized(f, fmt, h, w, STREAM_SIZE, "catrom") for f in frames]
    plain = e.upscale_yuv(frames[0], fmt, h, w)
    assert len({x.tobytes() for x in want}) == len(frames)
    v = r.VideoStream(e, fmt, h, w, slots=slots, size=STREAM_SIZE, filter="catrom")
    assert v.out_bytes == yuv_ref.frame_bytes(sub, *STREAM_SIZE)
    got = list(v.frames(frames))
    assert v.pending == 0 and len(got) == len(frames)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (slots, i)
    v.close()
    # a deep session, and a plain session made in the same process afterwards: the plain call's bytes
    case = ("422", "left", "bt709", "limited", 10)
    f16 = fmt16(case)
    deep_frames = smooth_frames16(901, case, 3, 13, 10)
    v = r.VideoStream(e, f16, 13, 10, slots=slots, size=(30, 21), srgb_space=True)
    for i, a in enumerate(v.frames(deep_frames)):
        assert a.tobytes() == e.upscale_yuv16_sized(deep_frames[i], f16, 13, 10, (30, 21), srgb_space=True).tobytes(), i
    v.close()
    v = r.VideoStream(e, fmt, h, w, slots=slots)
    assert v.out_bytes == plain.size and next(v.frames(frames[:1])).tobytes() == plain.tobytes()
    v.close()


def test_stream_recomputes_in_f32_when_a_frame_leaves_the_split_domain():
    """tests/test_gpu_video.py's fixture: parameters with which every frame leaves the split-half domain.  The sized session's frames
    are the exact-f32 call's, in order, and the context ends in exact f32; so does the synchronous sized call."""
    import domain_cases
    import rusty_sr_amd as r
    sub, siting, matrix, range_, h, w = STREAM
    fmt = fmt8(STREAM[:4])
    frames = smooth_frames8(900, sub, siting, matrix, range_, 5, h, w)
    p = domain_cases.wired("f", 5, 1.0)
    domain_cases._view(p, 3, "f_bias")[5] = 7e4
    exact = r.Engine(p, precision="f32")
    want = [exact.upscale_yuv_sized(f, fmt, h, w, STREAM_SIZE) for f in frames]
    exact.close()
    assert len({x.tobytes() for x in want}) == len(frames)
    e = r.Engine(p, precision="split_f16")
    assert e.upscale_yuv_sized(frames[0], fmt, h, w, STREAM_SIZE).tobytes() == want[0].tobytes()   # the synchronous call recomputes too
    e.check_domain()
    e.set_precision("split_f16")
    v = r.VideoStream(e, fmt, h, w, slots=3, size=STREAM_SIZE)
    got = list(v.frames(frames))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), i
    e.check_domain()                             # the word was cleared
    v.close()
    e.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(engines):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    e, bil = engines(), engines(graph="bilinear")
    down = r.downsample_net()
    L, INV = e._L, _lib.SR_E_INVALID
    h, w, f, oh, ow = 6, 10, 3, 11, 17
    case = ("420", "left", "bt709", "limited")
    fmt, f16 = fmt8(case), fmt16(case + (10,))
    frame = smooth_frames8(1, *case, 1, h, w)[0]
    frame16 = smooth_frames16(1, case + (10,), 1, h, w)[0]
    rgb = np.random.default_rng(3).random((1, h, w, 3), dtype=np.float32)
    out = np.full(8 << 20, 0xA5, np.uint8)
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    p_out, p_rgb, p_in = out.ctypes.data_as(u8p), C.c_void_p(rgb.ctypes.data), frame.ctypes.data_as(u8p)
    p_out16, p_in16 = out.ctypes.data_as(u16p), frame16.ctypes.data_as(u16p)
    LZ = _lib.SR_FILTER_LANCZOS3
    v = C.c_void_p(0)

    def resize(ctx=e._ctx, a=p_rgb, ff=C.byref(fmt), n=1, hh=h, ww=w, b=p_out, o_h=oh, o_w=ow, flt=LZ, flags=0):
        return L.sr_resize_to_yuv(ctx, a, ff, n, hh, ww, b, o_h, o_w, flt, flags)

    def resize16(ctx=e._ctx, a=p_rgb, ff=C.byref(f16), n=1, hh=h, ww=w, b=p_out16, o_h=oh, o_w=ow, flt=LZ, flags=0):
        return L.sr_resize_to_yuv16(ctx, a, ff, n, hh, ww, b, o_h, o_w, flt, flags)

    def up(ctx=e._ctx, a=p_in, ff=C.byref(fmt), n=1, hh=h, ww=w, b=p_out, o_h=oh, o_w=ow, flt=LZ, flags=0, members=1):
        return L.sr_upscale_yuv_sized(ctx, a, ff, n, hh, ww, b, o_h, o_w, flt, flags, members)

    def up16(ctx=e._ctx, a=p_in16, ff=C.byref(f16), n=1, hh=h, ww=w, b=p_out16, o_h=oh, o_w=ow, flt=LZ, flags=0, members=1):
        return L.sr_upscale_yuv16_sized(ctx, a, ff, n, hh, ww, b, o_h, o_w, flt, flags, members)

    def create(ctx=e._ctx, ff=C.byref(fmt), hh=h, ww=w, o_h=oh, o_w=ow, flt=LZ, flags=0, slots=3, members=1, o=C.byref(v)):
        return L.sr_video_create_sized(ctx, ff, hh, ww, o_h, o_w, flt, flags, slots, members, o)

    def create16(ctx=e._ctx, ff=C.byref(f16), hh=h, ww=w, o_h=oh, o_w=ow, flt=LZ, flags=0, slots=3, members=1, o=C.byref(v)):
        return L.sr_video_create16_sized(ctx, ff, hh, ww, o_h, o_w, flt, flags, slots, members, o)

    calls, sessions = (resize, resize16, up, up16), (create, create16)
    for call in calls:
        assert call(a=None) == INV and call(b=None) == INV and call(ff=None) == INV and call(ctx=None) == INV
        for n, hh, ww in ((0, h, w), (1, 0, w), (1, h, 0), (-1, h, w), (1, 2 ** 30, w), (1, h, 2 ** 30)):   # those of sr_upscale_yuv*
            assert call(n=n, hh=hh, ww=ww) == INV, (call.__name__, n, hh, ww)
    for call in calls + sessions:
        for o_h, o_w in ((0, ow), (oh, 0), (-3, ow), (oh, -1), (2 ** 30, ow), (oh, 2 ** 30), (2 ** 29, 2 ** 29)):   # sr_resize_dev's, and the side limit
            assert call(o_h=o_h, o_w=o_w) == INV, (call.__name__, o_h, o_w)
        for flt in (-1, 4, 1 << 20):
            assert call(flt=flt) == INV
        for flags in (2, 4, 0xFFFFFFFF):
            assert call(flags=flags) == INV
        for field in ("subsampling", "siting", "matrix", "range"):
            for bad in (-1, 3, 1 << 20):
                wrong8, wrong16 = fmt8(case), fmt16(case + (10,))
                setattr(wrong8, field, bad)
                setattr(wrong16, field, bad)
                assert call(ff=C.byref(wrong16 if "16" in call.__name__ else wrong8)) == INV
    wrong8 = fmt8(case)
    wrong8.subsampling = _lib.SR_YUV_422                    # 4:2:2 and BT.2020 are the deep struct's
    assert resize(ff=C.byref(wrong8)) == INV and up(ff=C.byref(wrong8)) == INV and create(ff=C.byref(wrong8)) == INV
    for depth in (8, 17, 0):
        wrong16 = fmt16(case + (10,))
        wrong16.depth = depth
        assert resize16(ff=C.byref(wrong16)) == INV and up16(ff=C.byref(wrong16)) == INV and create16(ff=C.byref(wrong16)) == INV
    odd = C.cast(C.c_void_p(out.ctypes.data + 1), u16p)     # deep frames are 2-byte aligned
    assert resize16(b=odd) == INV and up16(b=odd) == INV and up16(a=odd) == INV
    for call in (up, up16) + sessions:
        for members in (0, 256, 1 << 20):
            assert call(members=members) == INV
        for members in (0, 3, 0xFF):                        # members != 1 off sr_net
            assert call(ctx=bil._ctx, members=members) == INV
        assert call(ctx=down._ctx) == INV                   # the downsample graph has no composed call ...
    for call in sessions:
        assert call(ff=None) == INV and call(o=None) == INV and call(ctx=None) == INV
        for hh, ww in ((0, w), (h, 0), (2 ** 30, w)):
            assert call(hh=hh, ww=ww) == INV
        for slots in (0, 9, -1, 1 << 20):
            assert call(slots=slots) == INV
    assert not v.value and (out == 0xA5).all()
    assert resize(ctx=down._ctx) == _lib.SR_OK              # ... but resamples to a frame, like any context
    want = e.rgb_to_yuv(e.resize(rgb, (oh, ow)), fmt)
    assert out[:want.size].tobytes() == want.tobytes() and (out[want.size:] == 0xA5).all()
    down.close()
    # a workspace no device can hold is SR_E_NOMEM by arithmetic, before any launch; the context still serves
    # (frames of 3000 x 4 -> 1 x 2^22: small frames either side, an intermediate of 9000 x 2^22 x 12 bytes = 453 GB)
    out[:] = 0xA5
    tall = np.zeros(yuv_ref.frame_bytes("420", 3000, 4), np.uint8)
    assert yuv_ref.frame_bytes("420", 1, 2 ** 22) <= out.size
    assert up(a=tall.ctypes.data_as(u8p), hh=3000, ww=4, o_h=1, o_w=2 ** 22) == _lib.SR_E_NOMEM
    assert create(hh=3000, ww=4, o_h=1, o_w=2 ** 22) == _lib.SR_E_NOMEM
    assert not v.value and (out == 0xA5).all()
    good = e.upscale_yuv_sized(frame, fmt, h, w, (oh, ow))
    assert good.shape == (yuv_ref.frame_bytes("420", oh, ow),)
    # a sized session refuses row reuse and stays usable; a plain one takes it
    live = r.VideoStream(e, fmt, h, w, slots=2, size=(oh, ow))
    assert L.sr_video_set_reuse(live._v, _lib.SR_VIDEO_REUSE_ROWS) == INV
    assert L.sr_video_set_reuse(live._v, _lib.SR_VIDEO_REUSE_OFF) == _lib.SR_OK
    assert L.sr_video_set_reuse(live._v, 2) == INV
    live.submit(frame)
    assert live.receive().tobytes() == good.tobytes()
    live.close()
    with pytest.raises(r.SrError) as err:
        r.VideoStream(e, fmt, h, w, size=(oh, ow), reuse=True)
    assert err.value.status == INV
    plain = r.VideoStream(e, fmt, h, w, slots=2, reuse=True)
    plain.submit(frame)
    assert plain.receive().tobytes() == e.upscale_yuv(frame, fmt, h, w).tobytes()
    plain.close()
    # the host forms, through the binding
    for call in (lambda: e.upscale_yuv_sized(frame, fmt, h, w, (0, ow)), lambda: e.upscale_yuv_sized(frame, fmt, h, w, (oh, ow), filter=7),
                 lambda: e.upscale_yuv_sized(frame, fmt, h, w, (oh, ow), members=0), lambda: e.resize_to_yuv(rgb, fmt, (oh, -2)),
                 lambda: e.upscale_yuv16_sized(frame16, f16, h, w, (oh, 2 ** 30)), lambda: r.VideoStream(e, fmt, h, w, slots=0, size=(oh, ow)),
                 lambda: r.VideoStream(bil, fmt, h, w, members=3, size=(oh, ow))):
        with pytest.raises(r.SrError) as err:
            call()
        assert err.value.status == INV
    assert e.upscale_yuv_sized(frame, fmt, h, w, (oh, ow)).tobytes() == good.tobytes()


# ---- 5. the command line -----------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rusty_sr_amd", "bin", "rusty_sr")


def test_cli_video_sized(engines, tmp_path):
    from rusty_sr_amd.build import build_host
    from test_yuv_cpu import y4m_bytes
    build_host()
    e = engines()
    # --size, then --scale, on an 8-bit stream (small frames: BT.601 without --matrix)
    sub, siting, range_, h, w = "420", "left", "limited", 13, 17
    fmt = fmt8((sub, siting, "bt601", range_))
    frames = smooth_frames8(53, sub, siting, "bt601", range_, 4, h, w)
    lines = ["FRAME", "FRAME Ip", "FRAME XPTS=2", "FRAME"]
    stream = y4m_bytes("YUV4MPEG2 W17 H13 F25:1 Ip A1:1 C420mpeg2", frames, lines)

    def check(data, header, size, want_frames):
        head, got = split_y4m(data, len(want_frames[0]))
        assert head.decode() == header
        assert [g[0].decode() for g in got] == lines[:len(want_frames)]
        for i, g in enumerate(got):
            assert g[1] == want_frames[i], (size, i)

    want = [e.upscale_yuv_sized(f, fmt, h, w, (29, 40)).tobytes() for f in frames]
    res = subprocess.run([CLI, "video", "--size", "40x29", "--timing", "-", "-"], input=stream, capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr
    check(res.stdout, "YUV4MPEG2 W40 H29 F25:1 Ip A493:520 C420mpeg2", (29, 40), want)     # 1 17 29 : 1 13 40 = 493 : 520, coprime
    assert b"[timing] frames 4, " in res.stderr
    # --scale 2 is relative to the INPUT: 2x frames from the x3 weights; a uniform resize writes the A tag it read; one slot, files
    src, out = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(stream)
    want = [e.upscale_yuv_sized(f, fmt, h, w, (26, 34), "catrom", True).tobytes() for f in frames]
    res = subprocess.run([CLI, "video", "--scale", "2", "--filter", "catrom", "--resize-space=srgb", "--slots", "1", str(src), str(out)],
                         capture_output=True, timeout=120)
    assert res.returncode == 0 and res.stdout == b"", res.stderr
    check(out.read_bytes(), "YUV4MPEG2 W34 H26 F25:1 Ip A1:1 C420mpeg2", (26, 34), want)
    # --scale 1.5 rounds half up an axis: floor(17 1.5 + 0.5) = 26, floor(13 1.5 + 0.5) = 20; with -p bilinear and split_f16 it still runs
    bil = engines(graph="bilinear")
    want = [bil.upscale_yuv_sized(f, fmt, h, w, (20, 26)).tobytes() for f in frames[:2]]
    res = subprocess.run([CLI, "video", "-p", "bilinear", "--scale", "1.5", "-", "-"], input=y4m_bytes("YUV4MPEG2 W17 H13 C420mpeg2", frames[:2], lines[:2]),
                         capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr
    check(res.stdout, "YUV4MPEG2 W26 H20 C420mpeg2", (20, 26), want)
    # --depth auto on a C420p10 stream, with an ensemble
    case = ("420", "left", "bt601", "limited", 10)
    f16 = fmt16(case)
    deep = smooth_frames16(54, case, 3, 12, 16)
    stream16 = y4m_bytes("YUV4MPEG2 W16 H12 F30:1 A16:15 C420p10", [f.tobytes() for f in deep], lines[:3])
    want = [e.upscale_yuv16_sized(f, f16, 12, 16, (27, 32), members=0x03).tobytes() for f in deep]
    res = subprocess.run([CLI, "video", "--depth", "auto", "--size", "32x27", "--ensemble", "2", "-", "-"], input=stream16, capture_output=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    check(res.stdout, "YUV4MPEG2 W32 H27 F30:1 A6:5 C420p10", (27, 32), want)             # 16 16 27 : 15 12 32 = 6912 : 5760
    # without the options: the factor's frames and header, as before
    want = [e.upscale_yuv(f, fmt, h, w).tobytes() for f in frames]
    res = subprocess.run([CLI, "video", "-", "-"], input=stream, capture_output=True, timeout=120)
    assert res.returncode == 0, res.stderr
    check(res.stdout, "YUV4MPEG2 W51 H39 F25:1 Ip A1:1 C420mpeg2", (39, 51), want)
    # each refusal by name: status 2, nothing written
    for args, message in ((("--size", "8x8", "--scale", "2"), b"cannot be used with '--scale <S>'"),
                          (("--filter", "box"), b"<--size <WxH>|--scale <S>>"), (("--resize-space", "srgb"), b"<--size <WxH>|--scale <S>>"),
                          (("--reuse", "--size", "8x8"), b"'--reuse' cannot be used with '--size <WxH>'"),
                          (("--reuse", "--scale", "2"), b"'--reuse' cannot be used with '--scale <S>'")):
        res = subprocess.run([CLI, "video", *args, "-", "-"], input=stream, capture_output=True, timeout=120)
        assert res.returncode == 2 and message in res.stderr and res.stdout == b"", (args, res.stderr)
