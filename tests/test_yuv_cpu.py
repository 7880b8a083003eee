"""The colour rule of the video path on the CPU: tests/yuv_ref.py held to its own properties and to Pillow, the frame sizes, and the
ABI in its four places (header, ctypes table, Rust).  No GPU: the kernels are held to yuv_ref in tests/test_gpu_video.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yuv_ref
from conftest import ROOT

MATRICES, RANGES = tuple(yuv_ref.MATRICES), yuv_ref.RANGES
NEW = ("sr_yuv_frame_bytes", "sr_yuv_to_rgb_dev", "sr_rgb_to_yuv_dev", "sr_upscale_yuv_dev", "sr_upscale_yuv", "sr_video_create",
       "sr_video_acquire", "sr_video_submit", "sr_video_receive", "sr_video_pending", "sr_video_destroy")


def in_gamut_triples(matrix, range_, count, seed):
    """`count` 8-bit (Y, Cb, Cr) triples whose RGB lies strictly inside [0, 1], drawn from the range's nominal codes."""
    rng = np.random.default_rng(seed)
    k = yuv_ref.Rule(matrix, range_)
    out = np.empty((0, 3), np.uint8)
    while len(out) < count:
        y = rng.integers(int(k.ylim[0]), int(k.ylim[1]) + 1, 4 * count)
        c = rng.integers(int(k.clim[0]), int(k.clim[1]) + 1, (2, 4 * count))
        t = np.stack([y, c[0], c[1]], axis=1).astype(np.uint8)
        rgb = yuv_ref.yuv_to_rgb(yuv_ref.join(t[:, 0], t[:, 1], t[:, 2]), 1, len(t), "444", "center", matrix, range_)[0].astype(np.float64)
        keep = ((rgb > 0.0) & (rgb < 1.0)).all(axis=1)
        out = np.concatenate([out, t[keep]])
    return out[:count]


@pytest.mark.parametrize("range_", RANGES)
@pytest.mark.parametrize("matrix", MATRICES)
def test_444_round_trip_of_in_gamut_triples_is_the_identity(matrix, range_):
    """8-bit YCbCr -> f32 RGB -> 8-bit YCbCr at 4:4:4 returns every in-gamut triple: the f32 rounding of RGB (2^-24 relative) times the
    largest inverse coefficient times 255 is orders below the half level that would move a byte."""
    t = in_gamut_triples(matrix, range_, 90000, 7)
    frame = yuv_ref.join(t[:, 0], t[:, 1], t[:, 2])
    rgb = yuv_ref.yuv_to_rgb(frame, 1, len(t), "444", "center", matrix, range_)
    back = yuv_ref.rgb_to_yuv(rgb, "444", "center", matrix, range_)
    assert int((back != frame).sum()) == 0


@pytest.mark.parametrize("siting", yuv_ref.SITINGS)
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (5, 7), (8, 6), (13, 17)])
def test_constant_chroma_420_frames_round_trip_exactly(shape, siting):
    """A frame whose chroma planes are constant has the same chroma at every pixel under either siting and every clamped edge, so any
    luma plane with it in gamut comes back byte for byte -- at odd sizes too."""
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    (_, _), (ch, cw) = yuv_ref.plane_shapes("420", h, w)
    for matrix in MATRICES:
        for range_ in RANGES:
            for cb, cr in ((128, 128), (120, 140), (140, 118)):
                y = rng.integers(90, 160, (h, w)).astype(np.uint8)
                frame = yuv_ref.join(y, np.full((ch, cw), cb, np.uint8), np.full((ch, cw), cr, np.uint8))
                rgb = yuv_ref.yuv_to_rgb(frame, h, w, "420", siting, matrix, range_)
                assert ((rgb > 0) & (rgb < 1)).all()
                back = yuv_ref.rgb_to_yuv(rgb, "420", siting, matrix, range_)
                assert back.tobytes() == frame.tobytes(), (matrix, range_, cb, cr)


def test_chroma_upsampling_weights_and_siting():
    """The taps: weights sum to 16, a ramp stays a ramp in the interior, and the left siting puts sample j ON luma column 2j."""
    c = (np.arange(6)[None, :] * 10 + np.arange(4)[:, None] * 3).astype(np.uint8)
    for siting in yuv_ref.SITINGS:
        up = yuv_ref.upsample_chroma(c, 8, 12, siting)
        assert up.shape == (8, 12)
        assert (yuv_ref.upsample_chroma(np.full((4, 6), 77, np.uint8), 8, 12, siting) == 16 * 77).all()
        # interior columns: the horizontal step of the ramp is 10 per chroma sample, 5 per luma column = 80 in sixteenths
        assert (np.diff(up[:, 2:10], axis=1) == 80).all()
    left = yuv_ref.upsample_chroma(c, 8, 12, "left")
    centre = yuv_ref.upsample_chroma(c, 8, 12, "center")
    # vertically both are centred: row 2i is (C[i-1] + 3 C[i]) / 4
    assert (left[2, ::2] == 4 * (c[0].astype(int) + 3 * c[1].astype(int))).all()
    assert (centre[2, 2] == (c[0, 0] + 3 * c[0, 1]) * 1 + (c[1, 0] + 3 * c[1, 1]) * 3)
    # odd sizes clamp
    assert yuv_ref.upsample_chroma(c[:3, :4], 5, 7, "center").shape == (5, 7)


def test_subsampling_clamps_at_odd_sizes_and_nan_counts_as_zero():
    rgb = np.zeros((3, 3, 3), np.float32)
    rgb[2, 2] = 1.0
    for siting in yuv_ref.SITINGS:
        f = yuv_ref.rgb_to_yuv(rgb, "420", siting, "bt601", "full")
        y, cb, cr = yuv_ref.split(f, "420", 3, 3)
        assert y[2, 2] == 255 and y[0, 0] == 0 and cb.shape == (2, 2)
        assert cb[1, 1] == 128 and cr[1, 1] == 128      # the corner block is the white pixel four times over
    wild = np.array([[[np.nan, -1e30, 1e30], [np.inf, -np.inf, 0.5]]], np.float32)
    tame = np.array([[[0.0, 0.0, 1.0], [1.0, 0.0, 0.5]]], np.float32)
    for sub in yuv_ref.SUBSAMPLINGS:
        assert yuv_ref.rgb_to_yuv(wild, sub).tobytes() == yuv_ref.rgb_to_yuv(tame, sub).tobytes()


def test_against_pillow_full_range_601():
    """Pillow's convert("YCbCr") is full-range BT.601 at 4:4:4 in fixed point: the maximum difference is what can be compared (its
    rounding differs on about half the bytes), and it is at most one level, both ways."""
    from PIL import Image
    rng = np.random.default_rng(3)
    rgb8 = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    ours = yuv_ref.rgb_to_yuv(rgb8.astype(np.float32) / np.float32(255.0), "444", "center", "bt601", "full")
    theirs = np.array(Image.fromarray(rgb8).convert("YCbCr"))
    d = np.abs(np.stack(yuv_ref.split(ours, "444", 64, 96), axis=-1).astype(int) - theirs.astype(int))
    print("rgb -> ycbcr vs Pillow: max", d.max(), "share", (d != 0).mean())
    assert d.max() <= 1
    # the other way, on triples Pillow itself made (so they are in gamut up to its own rounding)
    back = np.array(Image.fromarray(theirs, "YCbCr").convert("RGB"))
    frame = yuv_ref.join(theirs[..., 0], theirs[..., 1], theirs[..., 2])
    mine = np.floor(yuv_ref.yuv_to_rgb(frame, 64, 96, "444", "center", "bt601", "full").astype(np.float64) * 255.0 + 0.5)
    d = np.abs(mine.astype(int) - back.astype(int))
    print("ycbcr -> rgb vs Pillow: max", d.max(), "share", (d != 0).mean())
    assert d.max() <= 1


def test_plane_sizes_and_frame_bytes():
    from rusty_sr_amd import YuvFormat, yuv_frame_bytes
    for h, w in ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (16, 12), (17, 13), (1080, 1920)):
        (_, _), (ch, cw) = yuv_ref.plane_shapes("420", h, w)
        assert (ch, cw) == (-(-h // 2), -(-w // 2))
        assert yuv_ref.frame_bytes("420", h, w) == h * w + 2 * ch * cw
        assert yuv_ref.frame_bytes("444", h, w) == 3 * h * w
        for sub in yuv_ref.SUBSAMPLINGS:
            for siting in yuv_ref.SITINGS:
                assert yuv_frame_bytes(YuvFormat.named(sub, siting, "bt709", "full"), h, w) == yuv_ref.frame_bytes(sub, h, w)
    good = YuvFormat.named()
    assert yuv_frame_bytes(good, 0, 4) == 0 and yuv_frame_bytes(good, 4, 0) == 0 and yuv_frame_bytes(good, -1, 4) == 0
    for field in ("subsampling", "siting", "matrix", "range"):
        for bad in (-1, 2, 1 << 20):
            fmt = YuvFormat.named()
            setattr(fmt, field, bad)
            assert yuv_frame_bytes(fmt, 4, 4) == 0, (field, bad)
    big = 2 ** 31 - 1
    assert yuv_frame_bytes(YuvFormat.named("444"), big, big) == 3 * big * big   # no 32-bit arithmetic


def test_entry_points_are_declared_and_exported():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust_host", "src", "srhip.rs")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert f"pub fn {name}(" in rust and f"pub fn {name}(" in md, name
    for name, val in re.findall(r"\b(SR_YUV_[A-Z0-9_]+) = (\d+)", header):
        assert getattr(_lib, name) == int(val), name
    assert C.sizeof(_lib.YuvFormat) == 16


def test_entry_points_without_a_context():
    """A null context (or session) is refused by every entry point before anything else is looked at."""
    from rusty_sr_amd import _lib
    L = _lib.lib()
    fmt = _lib.YuvFormat.named()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    INV = _lib.SR_E_INVALID
    assert L.sr_yuv_to_rgb_dev(None, p, C.byref(fmt), 1, 2, 2, p, None) == INV
    assert L.sr_rgb_to_yuv_dev(None, p, C.byref(fmt), 1, 2, 2, p, None) == INV
    assert L.sr_upscale_yuv_dev(None, p, C.byref(fmt), 1, 2, 2, p, 1, None) == INV
    assert L.sr_upscale_yuv(None, buf, C.byref(fmt), 1, 2, 2, buf, 1) == INV
    v = C.c_void_p(1)
    assert L.sr_video_create(None, C.byref(fmt), 2, 2, 3, 1, C.byref(v)) == INV and not v.value
    assert L.sr_video_acquire(None, C.byref(v)) == INV and L.sr_video_submit(None) == INV and L.sr_video_receive(None, C.byref(v)) == INV
    assert L.sr_video_pending(None) == -1
    L.sr_video_destroy(None)


def test_oracle_frames_are_well_conditioned(params):
    """The frames tests/test_gpu_video.py holds the composed call to the oracle on: through yuv_ref on both sides, the f32 oracle and
    its f64 build differ by at most one level on a share of the bytes below ORACLE_GATE of the cap the GPU is given, so the cap measures
    the kernels and not the reference's own rounding."""
    import test_gpu_video as tv
    for name, frame, h, w in tv.oracle_frames():
        a = tv.oracle_upscale(params["imagenet"], frame, h, w)
        b = tv.oracle_upscale(params["imagenet"], frame, h, w, f64=True)
        d = np.abs(a.astype(int) - b.astype(int))
        print(f"{name}: f32 against f64 oracle: {int((d != 0).sum())} of {d.size} bytes differ, max {d.max()}")
        assert a.size == yuv_ref.frame_bytes("420", 3 * h, 3 * w)
        assert d.max() <= 1 and (d != 0).mean() < tv.ORACLE_GATE * tv.ORACLE_CAP, name


# ---- the Y4M side of `rusty_sr video`: the header parser alone (a stand-alone program, also under ASan + UBSan) and through the CLI ----
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")
REFUSED_TAGS = ("C422", "C420paldv", "Cmono", "C420p10", "C444p12", "C422p16", "C420p16", "It", "Ib", "Im")


def y4m_bytes(header, frames, frame_lines=None):
    out = header.encode() + b"\n"
    for i, f in enumerate(frames):
        out += (frame_lines[i] if frame_lines else "FRAME").encode() + b"\n" + bytes(f)
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_header_parser_program(tmp_path, sanitize):
    import subprocess
    exe = str(tmp_path / ("y4m_header_san" if sanitize else "y4m_header"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "y4m_header.cpp"),
                           os.path.join(ROOT, "rusty_sr_amd", "host", "y4m.cpp"), "-o", exe])
    good = ["YUV4MPEG2 W17 H13 F25:1 Ip A1:1 C420mpeg2", "YUV4MPEG2 W16 H12 C444 XCOLORRANGE=FULL", "YUV4MPEG2 H2 W3", "YUV4MPEG2 W8 H8 C420",
            "YUV4MPEG2 W8 H8 F30:1 C420jpeg XYSCSS=420JPEG"]
    bad = ["", "YUV4MPEG", "YUV4MPEG2", "YUV4MPEG2W4 H4", "YUV4MPEG3 W4 H4", "YUV4MPEG2 W4", "YUV4MPEG2 H4", "YUV4MPEG2 W0 H4", "YUV4MPEG2 W4 H-4",
           "YUV4MPEG2 W4 H4 W5", "YUV4MPEG2 W16385 H4", "YUV4MPEG2 W4x H4", "YUV4MPEG2 W H4", "YUV4MPEG2 W4 H4 C420 C444", "YUV4MPEG2 W4 H4 Q1",
           "YUV4MPEG2 W4 H4 C"] + [f"YUV4MPEG2 W4 H4 {t}" for t in REFUSED_TAGS]
    res = subprocess.run([exe, *good, *bad], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().split("\n")
    assert lines[0] == "ok 17 13 420 left limited | YUV4MPEG2 W51 H39 F25:1 Ip A1:1 C420mpeg2"
    assert lines[1] == "ok 16 12 444 center full | YUV4MPEG2 W48 H36 C444 XCOLORRANGE=FULL"
    assert lines[2] == "ok 3 2 420 center limited | YUV4MPEG2 H6 W9"
    assert lines[3].startswith("ok 8 8 420 center limited") and lines[4].endswith("C420jpeg XYSCSS=420JPEG")
    for text, line in zip(bad, lines[len(good):len(good) + len(bad)]):
        assert line.startswith("refused "), (text, line)
    for tag, line in zip(REFUSED_TAGS, lines[len(good) + len(bad) - len(REFUSED_TAGS):len(good) + len(bad)]):
        assert f"'{tag}'" in line, (tag, line)
    rest = lines[len(good) + len(bad):]
    assert rest[:3] == ["length 1024 ok", "length 1025 refused", "length 100000 refused"] and rest[3].startswith("refused ")
    assert rest[4:14] == ["line 0 nl -> 1 0", "line 0 eof -> 0 0", "line 5 nl -> 1 5", "line 5 eof -> -1 5", "line 1024 nl -> 1 1024",
                          "line 1024 eof -> -1 1024", "line 1025 nl -> -1 1024", "line 1025 eof -> -1 1024", "line 70000 nl -> -1 1024",
                          "line 70000 eof -> -1 1024"]
    assert rest[15] == "frame lines: 1 1 0 0"


def _video(stdin_bytes, *args):
    import subprocess
    from rusty_sr_amd.build import build_host
    build_host()
    return subprocess.run([CLI, "video", *args], input=stdin_bytes, capture_output=True, timeout=120)


def test_cli_refuses_streams_and_arguments_before_touching_a_gpu():
    """Every refusal here is decided on the header or the arguments: exit 2 with the message on stderr and nothing on stdout, with or
    without a GPU in the machine."""
    frame = bytes(yuv_ref.frame_bytes("420", 4, 4))
    for tag in REFUSED_TAGS:
        res = _video(y4m_bytes(f"YUV4MPEG2 W4 H4 F25:1 {tag}", [frame]), "-", "-")
        assert res.returncode == 2 and f"'{tag}'" in res.stderr.decode() and res.stdout == b"", (tag, res.stderr)
    for stream in (b"", b"YUV4MPEG2 W4 H4", b"RIFF....AVI \n", b"YUV4MPEG2 W4\nFRAME\n", b"YUV4MPEG2 W0 H4\n", b"YUV4MPEG2 W4 H4 Cnonsense\n",
                   b"YUV4MPEG2 " + b"X" * 5000 + b"\n"):
        res = _video(stream, "-", "-")
        assert res.returncode == 2 and res.stderr.startswith(b"error: ") and res.stdout == b"", (stream[:40], res.stderr)
    good = y4m_bytes("YUV4MPEG2 W4 H4", [frame])
    res = _video(good, "--matrix", "nonsense", "-", "-")
    assert res.returncode == 2 and b"'nonsense' isn't a valid value for '--matrix <MATRIX>'" in res.stderr and res.stdout == b""
    res = _video(good, "-")
    assert res.returncode == 2 and b"required arguments were not provided" in res.stderr and res.stdout == b""
    for args in (("--slots", "0", "-", "-"), ("--slots", "9", "-", "-"), ("--ensemble", "3", "-", "-"), ("-p", "nothing", "-", "-"),
                 ("--precision", "f16", "-", "-"), ("-", "-", "-"), ("--ensemble", "2", "-p", "bilinear", "-", "-"), ("--nonsense", "-", "-")):
        res = _video(good, *args)
        assert res.returncode == 2 and res.stdout == b"", (args, res.stderr)
