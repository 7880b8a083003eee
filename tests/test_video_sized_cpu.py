"""Video at any size (include/srhip.h "Video at any size") without a GPU: the six entry points in the ABI's four places,
the header line `rusty_sr video --size / --scale` writes (sry4m::sized_header, under AddressSanitizer + UBSan as well), and the usage
refusals of the command line, which are decided before a device is touched.  The kernels and the calls themselves:
tests/test_gpu_video_sized.py."""
import inspect
import os
import re
import subprocess

import pytest

import yuv_ref
from conftest import ROOT

# name -> the number of its arguments
NEW = {"sr_resize_to_yuv": 11, "sr_resize_to_yuv16": 11, "sr_upscale_yuv_sized": 12, "sr_upscale_yuv16_sized": 12,
       "sr_video_create_sized": 11, "sr_video_create16_sized": 11}
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_entry_points_are_declared_exported_and_bound():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", _read("include", "srhip.h"), flags=re.S)
    rust = _read("rust_host", "src", "srhip.rs")
    md = _read("INTEGRATION.md")
    for name, nargs in NEW.items():
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, f"{name} is not declared in include/srhip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs, (name, args)
        assert not any("stream" in a for a in args), f"{name} takes a stream: it would need a row in tests/stream_order.py"
        assert hasattr(L, name), f"{name} is not exported"
        restype, argtypes = _lib.SYMBOLS[name]
        assert len(argtypes) == nargs, name
        for text in (rust, md):
            r = re.search(r"pub fn %s\(([^)]*)\) -> c_int;" % name, text)
            assert r and len(r.group(1).split(",")) == nargs, name
    assert "Video at any size" in _read("include", "srhip.h")
    # the deep calls take the deep format and 16-bit samples
    for name in NEW:
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, header, re.S).group(1)
        assert ("sr_yuv16_format" in m) == ("16" in name), name


def test_python_surface():
    import rusty_sr_amd as r
    from rusty_sr_amd.engine import Engine, VideoStream
    for name in ("resize_to_yuv", "resize_to_yuv16"):
        p = inspect.signature(getattr(Engine, name)).parameters
        assert list(p)[:4] == ["self", "x", "fmt", "size"] and p["filter"].default == "lanczos3" and p["srgb_space"].default is False
    for name in ("upscale_yuv_sized", "upscale_yuv16_sized"):
        p = inspect.signature(getattr(Engine, name)).parameters
        assert list(p)[:6] == ["self", "frames", "fmt", "h", "w", "size"] and p["members"].default == 1 and p["out"].default is None
    p = inspect.signature(VideoStream.__init__).parameters
    assert p["size"].default is None and p["filter"].default == "lanczos3" and p["srgb_space"].default is False and p["reuse"].default is False
    assert r.VideoStream is VideoStream


def test_the_kernel_is_built_and_resampling_yuv_shares_the_tile_helpers():
    from rusty_sr_amd import build
    assert "sr_resize_yuv.hip" in build.SOURCES and "sr_yuv_tile.h" in build.HEADERS
    kernel, yuv = _read("rusty_sr_amd", "csrc", "sr_resize_yuv.hip"), _read("rusty_sr_amd", "csrc", "sr_yuv.hip")
    for text in (kernel, yuv):
        assert '#include "sr_yuv_tile.h"' in text and "tile_store<" in text
        assert "atomic" not in re.sub(r"//[^\n]*", "", text)   # every sample belongs to one thread
    assert "fp contract(off)" in kernel


SIZED_CASES = [
    # header, ow, oh, expected
    ("YUV4MPEG2 W1920 H1080 F25:1 Ip A1:1 C420mpeg2", 3840, 2160, "YUV4MPEG2 W3840 H2160 F25:1 Ip A1:1 C420mpeg2"),        # uniform: the tag it read
    ("YUV4MPEG2 W720 H576 F25:1 Ip A16:15 C420jpeg", 1440, 1152, "YUV4MPEG2 W1440 H1152 F25:1 Ip A16:15 C420jpeg"),
    ("YUV4MPEG2 W720 H576 F25:1 Ip A16:15 C420jpeg", 1024, 576, "YUV4MPEG2 W1024 H576 F25:1 Ip A3:4 C420jpeg"),           # 16 720 576 : 15 576 1024
    ("YUV4MPEG2 W720 H576 A16:15", 1920, 1080, "YUV4MPEG2 W1920 H1080 A3:4"),                                             # SD PAL -> 1080p: 16 720 1080 : 15 576 1920
    ("YUV4MPEG2 W720 H576 A32:30", 1440, 1152, "YUV4MPEG2 W1440 H1152 A32:30"),                                          # uniform: not even reduced
    ("YUV4MPEG2 W720 H576 A32:30", 1024, 576, "YUV4MPEG2 W1024 H576 A3:4"),
    ("YUV4MPEG2 W17 H13 C444 XCOLORRANGE=FULL", 40, 9, "YUV4MPEG2 W40 H9 C444 XCOLORRANGE=FULL"),                         # no A tag
    ("YUV4MPEG2 H13 W17 A0:0", 40, 9, "YUV4MPEG2 H9 W40 A0:0"),                                                           # unknown, tag order kept
    ("YUV4MPEG2 W17 H13 A0:5", 40, 9, "YUV4MPEG2 W40 H9 A0:5"),
    ("YUV4MPEG2 W17 H13 A16", 40, 9, "YUV4MPEG2 W40 H9 A16"),                                                             # malformed: as written
    ("YUV4MPEG2 W17 H13 A:", 40, 9, "YUV4MPEG2 W40 H9 A:"),
    ("YUV4MPEG2 W17 H13 A", 40, 9, "YUV4MPEG2 W40 H9 A"),
    ("YUV4MPEG2 W17 H13 A16:15x", 40, 9, "YUV4MPEG2 W40 H9 A16:15x"),
    ("YUV4MPEG2 W17 H13 A-4:3", 40, 9, "YUV4MPEG2 W40 H9 A-4:3"),
    ("YUV4MPEG2 W17 H13 A4:3:2", 40, 9, "YUV4MPEG2 W40 H9 A4:3:2"),
    # nine-digit terms at the largest axes: 999999999 16384 16384 < 2^63
    ("YUV4MPEG2 W16384 H16384 A999999999:999999998", 16384, 16383, "YUV4MPEG2 W16384 H16383 A16382999983617:16383999967232"),
    ("YUV4MPEG2 W16384 H1 A999999999:1", 1, 16384, "YUV4MPEG2 W1 H16384 A268435455731564544:1"),
    # terms beyond 64-bit arithmetic pass through
    ("YUV4MPEG2 W16384 H16384 A99999999999999999999:3", 7, 5, "YUV4MPEG2 W7 H5 A99999999999999999999:3"),
    ("YUV4MPEG2 W16384 H16384 A999999999999999999:3", 7, 5, "YUV4MPEG2 W7 H5 A999999999999999999:3"),
    ("YUV4MPEG2 W8 H8 C420p10 A1:1", 12, 10, "YUV4MPEG2 W12 H10 C420p10 A5:6"),
]


def _expected_aspect(n, d, w, h, ow, oh):
    from math import gcd
    pn, pd = n * w * oh, d * h * ow
    g = gcd(pn, pd)
    return f"A{pn // g}:{pd // g}"


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_sized_header_program(tmp_path, sanitize):
    exe = str(tmp_path / ("y4m_header_sized_san" if sanitize else "y4m_header_sized"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "y4m_header_sized.cpp"),
                           os.path.join(ROOT, "rusty_sr_amd", "host", "y4m.cpp"), "-o", exe])
    args = [str(v) for case in SIZED_CASES for v in case[:3]]
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.rstrip("\n").split("\n")
    assert len(lines) == 2 * len(SIZED_CASES), res.stdout
    for (header, ow, oh, want), got, plain in zip(SIZED_CASES, lines[0::2], lines[1::2]):
        assert got == want, (header, ow, oh)
        # the expectation itself against the rule in integers: An:d -> (n W oh):(d H ow) over their gcd (a uniform resize: as read)
        a = re.fullmatch(r"A([1-9]\d{0,8}):([1-9]\d{0,8})", next((t for t in header.split() if t.startswith("A")), ""))
        if a:
            w0, h0 = int(re.search(r" W(\d+)", header).group(1)), int(re.search(r" H(\d+)", header).group(1))
            rule = a.group(0) if w0 * oh == h0 * ow else _expected_aspect(int(a.group(1)), int(a.group(2)), w0, h0, ow, oh)
            assert rule in got.split(), (header, ow, oh, rule)
        # scaled_header stays as it is: W and H times the factor, every other tag as written
        w, h = int(re.search(r" W(\d+)", header).group(1)), int(re.search(r" H(\d+)", header).group(1))
        assert plain == "  x3: " + header.replace(f"W{w}", f"W{3 * w}").replace(f"H{h}", f"H{3 * h}"), header


def _video(stdin_bytes, *args):
    from rusty_sr_amd.build import build_host
    build_host()
    return subprocess.run([CLI, "video", *args], input=stdin_bytes, capture_output=True, timeout=120)


def test_cli_usage_refusals_need_no_device():
    """Each by name, status 2, nothing on stdout -- decided on the arguments (and, for --scale's limit, on the header) alone."""
    frame = bytes(yuv_ref.frame_bytes("420", 4, 4))
    good = b"YUV4MPEG2 W4 H4\nFRAME\n" + frame
    cases = [
        (("--size", "8x8", "--scale", "2", "-", "-"), b"The argument '--size <WxH>' cannot be used with '--scale <S>'"),
        (("--filter", "box", "-", "-"), b"required arguments were not provided:\n    <--size <WxH>|--scale <S>>"),
        (("--resize-space", "srgb", "-", "-"), b"required arguments were not provided:\n    <--size <WxH>|--scale <S>>"),
        (("--reuse", "--size", "8x8", "-", "-"), b"The argument '--reuse' cannot be used with '--size <WxH>'"),
        (("--scale", "2", "--reuse", "-", "-"), b"The argument '--reuse' cannot be used with '--scale <S>'"),
        (("--size", "8", "-", "-"), b"'8' isn't a valid value for '--size <WxH>'"),
        (("--size", "0x8", "-", "-"), b"'0x8' isn't a valid value for '--size <WxH>'"),
        (("--size", "16385x8", "-", "-"), b"'16385x8' isn't a valid value for '--size <WxH>'\n\t[two whole numbers, 1..16384 each: 3840x2160]"),
        (("--size=8x", "-", "-"), b"'8x' isn't a valid value for '--size <WxH>'"),
        (("--scale", "-1", "-", "-"), b"'-1' isn't a valid value for '--scale <S>'\n\t[a positive decimal: 1.5]"),
        (("--scale", "0", "-", "-"), b"'0' isn't a valid value for '--scale <S>'"),
        (("--scale", "1e3", "-", "-"), b"'1e3' isn't a valid value for '--scale <S>'"),
        (("--scale", "5000", "-", "-"), b"'5000' isn't a valid value for '--scale <S>'\n\t[the output would exceed 16384 pixels on an axis]"),
        (("--size", "8x8", "--filter", "sinc", "-", "-"), b"'sinc' isn't a valid value for '--filter <FILTER>'\n\t[values: box, catrom, lanczos3, triangle]"),
        (("--size", "8x8", "--resize-space", "lab", "-", "-"), b"'lab' isn't a valid value for '--resize-space <SPACE>'\n\t[values: linear, srgb]"),
        (("--size",), b"The argument '--size <WxH>' requires a value but none was supplied"),
        (("--scale",), b"The argument '--scale <S>' requires a value but none was supplied"),
    ]
    for args, message in cases:
        res = _video(good, *args)
        assert res.returncode == 2 and message in res.stderr and res.stdout == b"", (args, res.stderr)
        assert res.stderr.startswith(b"error: ")
    # the option lines are in the help, and the image command's parsers are the ones used
    res = _video(b"", "--help")
    assert res.returncode == 0
    for line in (b"--size <WxH>", b"--scale <S>", b"--filter <FILTER>", b"--resize-space <SPACE>"):
        assert line in res.stderr
    main = _read("rusty_sr_amd", "host", "main.cpp")
    video = main[main.index("int run_video("):main.index("int main(")]
    assert "parse_size(" in video and "parse_scale(" in video and "scaled_axis(" in video and "sized_header(" in video
