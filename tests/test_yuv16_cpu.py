"""The colour rule of the deep video path on the CPU: tests/yuv16_ref.py held to its own properties and to the 8-bit rule (yuv_ref), the
frame sizes, the ABI in its four places (header, ctypes table, Rust), the `deep` overload of the Y4M header parser (a
stand-alone program, also under ASan + UBSan) and the refusals `rusty_sr video` decides before it touches a GPU.  No GPU: the kernels are
held to yuv16_ref in tests/test_gpu_video_deep.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import yuv16_ref
import yuv_ref
from conftest import ROOT

MATRICES, RANGES = tuple(yuv16_ref.MATRICES), yuv16_ref.RANGES
NEW = ("sr_yuv16_frame_bytes", "sr_yuv16_to_rgb_dev", "sr_rgb_to_yuv16_dev", "sr_upscale_yuv16_dev", "sr_upscale_yuv16", "sr_video_create16")
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")
DEEP_TAGS = tuple(f"C{sub}p{d}" for sub in ("420", "422", "444") for d in (9, 10, 12, 14, 16))


def in_gamut_triples(matrix, range_, depth, count, seed):
    """`count` (Y, Cb, Cr) triples of `depth` bits whose RGB lies strictly inside [0, 1], drawn from the range's nominal codes."""
    rng = np.random.default_rng(seed)
    k = yuv16_ref.Rule(matrix, range_, depth)
    out = np.empty((0, 3), np.uint16)
    while len(out) < count:
        y = rng.integers(int(k.ylim[0]), int(k.ylim[1]) + 1, 4 * count)
        c = rng.integers(int(k.clim[0]), int(k.clim[1]) + 1, (2, 4 * count))
        t = np.stack([y, c[0], c[1]], axis=1).astype(np.uint16)
        rgb = yuv16_ref.yuv_to_rgb(yuv16_ref.join(t[:, 0], t[:, 1], t[:, 2]), 1, len(t), "444", "center", matrix, range_, depth)[0].astype(np.float64)
        keep = ((rgb > 0.0) & (rgb < 1.0)).all(axis=1)
        out = np.concatenate([out, t[keep]])
    return out[:count]


@pytest.mark.parametrize("depth", [9, 10, 12, 14, 16])
def test_444_round_trip_of_in_gamut_triples_is_the_identity(depth):
    """d-bit YCbCr -> f32 RGB -> d-bit YCbCr at 4:4:4 returns every in-gamut triple, at every depth, matrix and range: at 16 bits the f32
    rounding of RGB (2^-25 of at most 1) times the largest forward gain (kc ir 2 (1 - Kr) = kc < 2^16) stays below 2^-9 of a level."""
    for matrix in MATRICES:
        for range_ in RANGES:
            t = in_gamut_triples(matrix, range_, depth, 40000, depth)
            frame = yuv16_ref.join(t[:, 0], t[:, 1], t[:, 2])
            rgb = yuv16_ref.yuv_to_rgb(frame, 1, len(t), "444", "center", matrix, range_, depth)
            back = yuv16_ref.rgb_to_yuv(rgb, "444", "center", matrix, range_, depth)
            assert int((back != frame).sum()) == 0, (matrix, range_, depth)


@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_limited_range_is_the_8_bit_rule_scaled_by_a_power_of_two(matrix, depth):
    """In limited range every constant of the deep rule is the 8-bit rule's times 2^(d - 8), so the deep rule on code 2^(d - 8) gives the
    8-bit rule's f32 RGB bit for bit: every code, every chroma tap, both sitings, odd sizes."""
    rng = np.random.default_rng(depth)
    s = 1 << (depth - 8)
    for sub, siting, h, w in (("420", "center", 7, 9), ("420", "left", 6, 11), ("444", "center", 5, 5)):
        frame8 = rng.integers(0, 256, yuv_ref.frame_bytes(sub, h, w), dtype=np.uint8)
        a = yuv_ref.yuv_to_rgb(frame8, h, w, sub, siting, matrix, "limited")
        b = yuv16_ref.yuv_to_rgb(frame8.astype(np.uint16) * s, h, w, sub, siting, matrix, "limited", depth)
        assert a.tobytes() == b.tobytes(), (sub, siting)
    codes = np.arange(256, dtype=np.uint8)
    grid = np.stack(np.meshgrid(codes[::5], codes[::3], codes[::7], indexing="ij"), axis=-1).reshape(-1, 3)
    f8 = yuv_ref.join(grid[:, 0], grid[:, 1], grid[:, 2])
    a = yuv_ref.yuv_to_rgb(f8, 1, len(grid), "444", "center", matrix, "limited")
    b = yuv16_ref.yuv_to_rgb(f8.astype(np.uint16) * s, 1, len(grid), "444", "center", matrix, "limited", depth)
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("siting", yuv16_ref.SITINGS)
@pytest.mark.parametrize("sub", ["420", "422"])
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (5, 7), (8, 6), (13, 17)])
def test_constant_chroma_frames_round_trip_exactly(shape, sub, siting):
    """A frame whose chroma planes are constant has the same chroma at every pixel under either siting and every clamped edge, so any
    luma plane with it in gamut comes back sample for sample -- at odd sizes too, at 4:2:0 and 4:2:2."""
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)
    (_, _), (ch, cw) = yuv16_ref.plane_shapes(sub, h, w)
    for matrix, range_, depth in (("bt601", "limited", 10), ("bt709", "full", 12), ("bt2020", "limited", 16), ("bt2020", "full", 10)):
        s = 1 << (depth - 8)
        for cb, cr in ((128, 128), (120, 140), (140, 118)):
            y = (rng.integers(90 * s, 160 * s, (h, w))).astype(np.uint16)
            frame = yuv16_ref.join(y, np.full((ch, cw), cb * s + 1, np.uint16), np.full((ch, cw), cr * s + 1, np.uint16))
            rgb = yuv16_ref.yuv_to_rgb(frame, h, w, sub, siting, matrix, range_, depth)
            assert ((rgb > 0) & (rgb < 1)).all()
            back = yuv16_ref.rgb_to_yuv(rgb, sub, siting, matrix, range_, depth)
            assert back.tobytes() == frame.tobytes(), (matrix, range_, depth, cb, cr)


def test_422_taps_and_subsampling():
    """4:2:2: the horizontal taps alone -- weights sum to 4, no vertical tap, the left siting puts sample j ON luma column 2j -- and the
    two subsampling filters at an odd width."""
    c = (np.arange(6)[None, :] * 10 + np.arange(4)[:, None] * 3).astype(np.uint16)
    for siting in yuv16_ref.SITINGS:
        up = yuv16_ref.upsample_chroma_422(c, 12, siting)
        assert up.shape == (4, 12)
        assert (yuv16_ref.upsample_chroma_422(np.full((4, 6), 777, np.uint16), 12, siting) == 4 * 777).all()
        assert (np.diff(up[:, 2:10], axis=1) == 20).all()                     # the ramp: 5 a luma column, in quarters
        assert (np.diff(up, axis=0) == 12).all()                              # rows are independent: the plane's own row step
    assert (yuv16_ref.upsample_chroma_422(c, 12, "left")[:, ::2] == 4 * c.astype(int)).all()
    assert yuv16_ref.upsample_chroma_422(c[:, :4], 7, "center").shape == (4, 7)
    rgb = np.zeros((2, 3, 3), np.float32)
    rgb[:, 2] = 1.0
    for siting in yuv16_ref.SITINGS:
        y, cb, cr = yuv16_ref.split(yuv16_ref.rgb_to_yuv(rgb, "422", siting, "bt709", "full", 10), "422", 2, 3)
        assert cb.shape == (2, 2) and (y[:, 2] == 1023).all() and (y[:, 0] == 0).all()
        assert (cb[:, 1] == 512).all() and (cr[:, 1] == 512).all()          # the last block is the white column over and over
        assert (cb[:, 0] == 512).all()                                         # black and black: grey chroma
    wild = np.array([[[np.nan, -1e30, 1e30], [np.inf, -np.inf, 0.5]]], np.float32)
    tame = np.array([[[0.0, 0.0, 1.0], [1.0, 0.0, 0.5]]], np.float32)
    for sub in yuv16_ref.SUBSAMPLINGS:
        assert yuv16_ref.rgb_to_yuv(wild, sub).tobytes() == yuv16_ref.rgb_to_yuv(tame, sub).tobytes()


def test_codes_are_taken_as_stored():
    """Nothing is masked: a Cb of 1536 in a 10-bit stream is the number 1536 (blue driven into the clamp), not 512 (grey)."""
    frame = yuv16_ref.join([[502, 502]], [[1536, 512]], [[512, 512]])
    rgb = yuv16_ref.yuv_to_rgb(frame, 1, 2, "444", "center", "bt709", "limited", 10)
    assert rgb[0, 0, 2] == 1.0 and rgb[0, 0, 0] == rgb[0, 1, 0] == np.float32(0.5) and rgb[0, 0, 1] < 0.3
    assert (rgb[0, 1] == np.float32(0.5)).all()


def test_plane_sizes_and_frame_bytes():
    from rusty_sr_amd import Yuv16Format, yuv16_frame_bytes
    for h, w in ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (16, 12), (17, 13), (1080, 1920)):
        assert yuv16_ref.plane_shapes("420", h, w)[1] == (-(-h // 2), -(-w // 2))
        assert yuv16_ref.plane_shapes("422", h, w)[1] == (h, -(-w // 2))
        assert yuv16_ref.plane_shapes("444", h, w)[1] == (h, w)
        for sub in yuv16_ref.SUBSAMPLINGS:
            for siting in yuv16_ref.SITINGS:
                for depth in (9, 10, 16):
                    assert yuv16_frame_bytes(Yuv16Format.named(sub, siting, "bt2020", "full", depth), h, w) == yuv16_ref.frame_bytes(sub, h, w)
    assert yuv16_ref.frame_bytes("420", 1080, 1920) == 2 * 1080 * 1920 * 3 // 2 and yuv16_ref.frame_bytes("422", 3, 5) == 2 * (15 + 2 * 9)
    good = Yuv16Format.named()
    assert yuv16_frame_bytes(good, 0, 4) == 0 and yuv16_frame_bytes(good, 4, 0) == 0 and yuv16_frame_bytes(good, -1, 4) == 0
    for field, bads in (("subsampling", (-1, 3, 1 << 20)), ("siting", (-1, 2, 1 << 20)), ("matrix", (-1, 3, 1 << 20)), ("range", (-1, 2, 1 << 20)),
                        ("depth", (-1, 0, 8, 17, 32, 1 << 20))):
        for bad in bads:
            fmt = Yuv16Format.named()
            setattr(fmt, field, bad)
            assert yuv16_frame_bytes(fmt, 4, 4) == 0, (field, bad)
    big = 2 ** 30
    assert yuv16_frame_bytes(Yuv16Format.named("444"), big, big) == 6 * big * big   # no 32-bit arithmetic
    assert yuv16_frame_bytes(Yuv16Format.named("444"), 2 ** 31 - 1, 2 ** 31 - 1) == 0  # ... and no 64-bit wrap: beyond size_t is no frame


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
    found = dict(re.findall(r"\b(SR_YUV_[A-Z0-9_]+) = (\d+)", header))
    assert found["SR_YUV_422"] == "2" and found["SR_YUV_BT2020"] == "2"
    for name, val in found.items():
        assert getattr(_lib, name) == int(val), name
    assert C.sizeof(_lib.Yuv16Format) == 20 and C.sizeof(_lib.YuvFormat) == 16
    assert re.search(r"struct sr_yuv16_format \{ int32_t subsampling, siting, matrix, range, depth; \}", header)
    assert "pub struct SrYuv16Format" in rust and "pub depth: i32" in rust


def test_entry_points_without_a_context():
    """A null context is refused by every new entry point before anything else is looked at."""
    from rusty_sr_amd import _lib
    L = _lib.lib()
    fmt = _lib.Yuv16Format.named()
    buf = (C.c_uint16 * 64)()
    p = C.cast(buf, C.c_void_p)
    INV = _lib.SR_E_INVALID
    assert L.sr_yuv16_to_rgb_dev(None, p, C.byref(fmt), 1, 2, 2, p, None) == INV
    assert L.sr_rgb_to_yuv16_dev(None, p, C.byref(fmt), 1, 2, 2, p, None) == INV
    assert L.sr_upscale_yuv16_dev(None, p, C.byref(fmt), 1, 2, 2, p, 1, None) == INV
    assert L.sr_upscale_yuv16(None, buf, C.byref(fmt), 1, 2, 2, buf, 1) == INV
    v = C.c_void_p(1)
    assert L.sr_video_create16(None, C.byref(fmt), 2, 2, 3, 1, C.byref(v)) == INV and not v.value


# ---- the Y4M side of `rusty_sr video --depth auto`: the header parser's deep overload alone, and the CLI's refusals ----
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_deep_header_parser_program(tmp_path, sanitize):
    exe = str(tmp_path / ("y4m_header_deep_san" if sanitize else "y4m_header_deep"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "y4m_header_deep.cpp"),
                           os.path.join(ROOT, "rusty_sr_amd", "host", "y4m.cpp"), "-o", exe])
    good = [f"YUV4MPEG2 W17 H13 F25:1 Ip {t}" for t in DEEP_TAGS] + ["YUV4MPEG2 W16 H12 C444p12 XCOLORRANGE=FULL", "YUV4MPEG2 H2 W3",
                                                                   "YUV4MPEG2 W8 H8 C420mpeg2", "YUV4MPEG2 W8 H8 C444"]
    bad = [f"YUV4MPEG2 W4 H4 {t}" for t in ("C422", "Cmono", "Cmono16", "C420paldv", "It", "Ib", "Im", "C420p8", "C420p11", "C420p", "C420p100",
                                            "C411p10", "C420jpegp10", "C420P10", "C420p10x", "Cp10")] + ["YUV4MPEG2 W4 H4 C420p10 C444p10"]
    res = subprocess.run([exe, *good, *bad, "--", *[f"YUV4MPEG2 W4 H4 {t}" for t in DEEP_TAGS], "YUV4MPEG2 W4 H4 C420mpeg2"],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr)
    lines = res.stdout.strip().split("\n")
    for tag, line in zip(DEEP_TAGS, lines):
        sub, depth = tag[1:4], int(tag[5:])
        siting = "center" if sub == "444" else "left"
        assert line == f"ok 17 13 {sub} {siting} limited {depth} | YUV4MPEG2 W51 H39 F25:1 Ip {tag}", line
    k = len(DEEP_TAGS)
    assert lines[k] == "ok 16 12 444 center full 12 | YUV4MPEG2 W48 H36 C444p12 XCOLORRANGE=FULL"
    assert lines[k + 1] == "ok 3 2 420 center limited 8 | YUV4MPEG2 H6 W9"
    assert lines[k + 2].startswith("ok 8 8 420 left limited 8 |") and lines[k + 3].startswith("ok 8 8 444 center limited 8 |")
    for text, line in zip(bad, lines[len(good):len(good) + len(bad)]):
        assert line.startswith("refused "), (text, line)
        tag = text.split()[3]
        assert f"'{tag}'" in line or "more than one C tag" in line, (text, line)
    rest = lines[len(good) + len(bad):]
    for tag, line in zip(DEEP_TAGS, rest):                                   # deep false: every deep tag is still refused by name
        assert line.startswith("refused ") and f"'{tag}'" in line, (tag, line)
    assert rest[k].startswith("ok 4 4 420 left limited 8 |")
    m = re.fullmatch(r"prefixes and mutations: (\d+) accepted, (\d+) refused, (\d+) deep", rest[k + 1])
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0 and int(m.group(3)) >= 3, rest[k + 1]


def _cli(stdin_bytes, *args):
    from rusty_sr_amd.build import build_host
    build_host()
    return subprocess.run([CLI, *args], input=stdin_bytes, capture_output=True, timeout=120)


def test_cli_refuses_the_new_options_before_touching_a_gpu():
    """Every refusal here is decided on the arguments or the header: exit 2, the message on stderr naming what is wrong, nothing on
    stdout, with or without a GPU in the machine."""
    from test_yuv_cpu import y4m_bytes
    frame8 = bytes(yuv_ref.frame_bytes("420", 4, 4))
    eight = y4m_bytes("YUV4MPEG2 W4 H4 F25:1 C420mpeg2", [frame8])
    for args, word in ((("--depth", "nonsense"), b"--depth"), (("--depth", "16"), b"--depth"), (("--depth=10", ), b"--depth"),
                       (("--depth", ), b"--depth"), (("--matrix", "bt2020"), b"--matrix"), (("--siting", "left"), b"--siting"),
                       (("--depth", "auto", "--matrix", "bt2020"), b"--matrix"), (("--depth", "auto", "--siting", "left"), b"--siting"),
                       (("--depth", "auto", "--siting", "nonsense"), b"--siting"), (("--siting", "nonsense"), b"--siting")):
        res = _cli(eight, "video", *args, "-", "-")
        assert res.returncode == 2 and word in res.stderr and res.stdout == b"", (args, res.stderr)
    for tag in ("C422", "Cmono16", "It", "Cmono", "C420paldv"):
        res = _cli(y4m_bytes(f"YUV4MPEG2 W4 H4 F25:1 {tag}", [frame8]), "video", "--depth", "auto", "-", "-")
        assert res.returncode == 2 and f"'{tag}'" in res.stderr.decode() and res.stdout == b"", (tag, res.stderr)
    for tag in DEEP_TAGS:                                                       # without the option a deep stream is refused as before
        res = _cli(y4m_bytes(f"YUV4MPEG2 W4 H4 F25:1 {tag}", [frame8]), "video", "-", "-")
        assert res.returncode == 2 and f"'{tag}'" in res.stderr.decode() and res.stdout == b"", (tag, res.stderr)
    for sub in ("train", "validate"):
        res = _cli(b"", sub, "--depth", "auto", "a", "b")
        assert res.returncode == 2 and b"--depth" in res.stderr and res.stdout == b"", (sub, res.stderr)
    res = _cli(b"", "video", "--help")
    assert res.returncode == 0 and b"--depth <BITS>" in res.stderr and b"--siting <SITING>" in res.stderr and b"bt2020" in res.stderr
