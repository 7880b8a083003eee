"""Deep colour without a GPU: the properties of the rule (tests/deep_ref.py), the 16-bit decode path and the two encoders of the host
codecs (rusty_sr_amd/host) against files this test writes and reads itself, the sanitizer program on mangled 16-bit files, the ABI in
its four places, and the CLI's refusals, which come before a device is touched."""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deep_ref
from conftest import ROOT

PNGLIB = os.path.join(ROOT, "rusty_sr_amd", "libsrpng.so")
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")
NAMES = ("sr_u16_to_f32_dev", "sr_f32_to_u16_dev", "sr_upscale_u16_dev", "sr_upscale_u16", "sr_upscale_u16_border_dev",
         "sr_upscale_u16_border", "sr_upscale_u16_sized_dev", "sr_upscale_u16_sized")
ARITY = (8, 8, 10, 9, 12, 11, 14, 13)
SIZES = ((1, 1), (5, 7), (33, 17))      # (w, h)
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}     # PNG colour type -> channels


# ---- 1. the rule ---------------------------------------------------------------------------------------------------------------------
def test_every_level_round_trips():
    k = np.arange(65536, dtype=np.uint16)
    for c in (1, 2, 3, 4):
        px = np.repeat(k[:, None], c, axis=1)
        x = deep_ref.to_f32(px)
        assert x.shape == (65536, 3) and x.dtype == np.float32
        assert (deep_ref.quantise(x, 3) == k[:, None]).all()
        assert (deep_ref.quantise(x, 1)[:, 0] == k).all()           # ... through the grey mean
        q4 = deep_ref.quantise(x, 4)
        assert (q4[:, :3] == k[:, None]).all() and (q4[:, 3] == 65535).all()
    rgb = np.stack([k, k[::-1], np.roll(k, 777)], axis=1)
    assert (deep_ref.quantise(deep_ref.to_f32(rgb)) == rgb).all()
    rgba = np.concatenate([rgb, np.full((65536, 1), 123, np.uint16)], axis=1)
    assert deep_ref.to_f32(rgba).tobytes() == deep_ref.to_f32(rgb).tobytes()       # alpha is dropped
    la = np.stack([k, k[::-1]], axis=1)
    assert deep_ref.to_f32(la).tobytes() == deep_ref.to_f32(k[:, None]).tobytes()


def test_promoted_bytes_feed_the_network_what_the_8_bit_path_feeds_it():
    b = np.arange(256)
    wide = deep_ref.to_f32((b * 257).astype(np.uint16)[:, None])[:, 0]
    assert wide.tobytes() == (b.astype(np.float32) / np.float32(255.0)).tobytes()


def test_quantise_is_monotone_clamps_and_sends_nan_to_zero():
    F = np.float32
    rng = np.random.default_rng(3)
    v = np.sort(np.concatenate([rng.random(200000, dtype=F) * F(1.4) - F(0.2), np.arange(65536, dtype=F) / F(65535.0),
                                ((np.arange(65536) + 0.5) / 65535.0).astype(F)]))
    q = deep_ref.quantise_values(v).astype(np.int64)
    assert (np.diff(q) >= 0).all() and q[0] == 0 and q[-1] == 65535
    odd = np.array([np.nan, -np.inf, -1e30, -1.0, -1e-9, -0.0, 0.0, 1e-45, 1.0, 1.0000001, 2.0, 3e38, np.inf], dtype=F)
    assert deep_ref.quantise_values(odd).tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 65535, 65535, 65535, 65535, 65535]
    assert deep_ref.quantise(np.array([[np.nan, 1.0, 1.0]], F), 1).tolist() == [[0]]       # a NaN in the mean is a NaN
    assert deep_ref.quantise(np.array([[0.25, 0.5, 0.75]], F), 1).tolist() == [[32768]]


# ---- 2. the codecs -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    from rusty_sr_amd.build import build_host
    build_host()
    L = C.CDLL(PNGLIB)
    u8pp, u16p, ip = C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint16), C.POINTER(C.c_int)
    L.srpng_decode_any_rgba8.argtypes = [C.c_char_p, ip, ip, u8pp]
    L.srpng_decode_any_u16.argtypes = [C.c_char_p, ip, ip, ip, ip, C.POINTER(u16p)]
    L.srpng_encode_png_u16.argtypes = [C.c_char_p, u16p, C.c_int, C.c_int, C.c_int]
    L.srpng_encode_any_u16.argtypes = L.srpng_encode_png_u16.argtypes
    L.srpng_free.argtypes = [C.c_void_p]

    class Codec:
        @staticmethod
        def decode8(path):
            w, h, p = C.c_int(), C.c_int(), C.POINTER(C.c_uint8)()
            assert L.srpng_decode_any_rgba8(str(path).encode(), C.byref(w), C.byref(h), C.byref(p)) == 0
            a = np.ctypeslib.as_array(p, (h.value, w.value, 4)).copy()
            L.srpng_free(p)
            return a

        @staticmethod
        def decode16(path):
            """-> (samples (h, w, channels), bits), or None where the file is refused"""
            w, h, c, bits, p = C.c_int(), C.c_int(), C.c_int(), C.c_int(), u16p()
            if L.srpng_decode_any_u16(str(path).encode(), C.byref(w), C.byref(h), C.byref(c), C.byref(bits), C.byref(p)) != 0:
                return None
            a = np.ctypeslib.as_array(p, (h.value, w.value, c.value)).copy()
            L.srpng_free(p)
            return a, bits.value

        @staticmethod
        def encode(path, px, png_only=False):
            px = np.ascontiguousarray(px, dtype=np.uint16)
            h, w, c = px.shape
            fn = L.srpng_encode_png_u16 if png_only else L.srpng_encode_any_u16
            return fn(str(path).encode(), px.ctypes.data_as(u16p), c, w, h)
    return Codec


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))   # x0, y0, dx, dy


def scanlines(px):
    """(rows, w, c) uint16 -> the filtered scanlines, high byte first: filter None on even rows, Sub on odd ones"""
    rows, w, c = px.shape
    out = b""
    for y in range(rows):
        raw = np.frombuffer(px[y].astype(">u2").tobytes(), np.uint8).astype(np.int32)
        if y % 2 == 0:
            out += b"\x00" + raw.astype(np.uint8).tobytes()
        else:
            left = np.concatenate([np.zeros(2 * c, np.int32), raw[:-2 * c]])
            out += b"\x01" + ((raw - left) & 255).astype(np.uint8).tobytes()
    return out


def write_png16(px, ctype, interlace=False):
    h, w, c = px.shape
    assert c == CHANNELS[ctype] and px.dtype == np.uint16
    if interlace:
        body = b"".join(scanlines(px[y0::dy, x0::dx]) for x0, y0, dx, dy in ADAM7 if px[y0::dy, x0::dx].size)
    else:
        body = scanlines(px)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, ctype, 0, 0, int(interlace)))
            + chunk(b"IDAT", zlib.compress(body)) + chunk(b"IEND", b""))


def read_png(data):
    """A small PNG reader (non-interlaced; inflate and the five filters) -> (samples (h, w, c), depth, colour type)"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    w, h, depth, ctype, _, _, interlace = hdr
    assert interlace == 0 and depth in (8, 16)
    c = CHANNELS[ctype]
    bpp, stride = c * depth // 8, w * c * depth // 8
    raw = zlib.decompress(idat)
    assert len(raw) == h * (stride + 1)
    prev, rows = bytearray(stride), []
    for y in range(h):
        ft, line = raw[y * (stride + 1)], bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        for i in range(stride):
            a = line[i - bpp] if i >= bpp else 0
            b, cc = prev[i], (prev[i - bpp] if i >= bpp else 0)
            if ft == 1:
                line[i] = (line[i] + a) & 255
            elif ft == 2:
                line[i] = (line[i] + b) & 255
            elif ft == 3:
                line[i] = (line[i] + (a + b) // 2) & 255
            elif ft == 4:
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                line[i] = (line[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else cc)) & 255
            else:
                assert ft == 0
        rows.append(bytes(line))
        prev = line
    px = np.frombuffer(b"".join(rows), ">u2" if depth == 16 else np.uint8).reshape(h, w, c)
    return px.astype(np.uint16 if depth == 16 else np.uint8), depth, ctype


def picture16(seed, w, h, c):
    """noise with both bytes live, a ramp row and a row inside one 8-bit level"""
    px = np.random.default_rng(seed).integers(0, 65536, (h, w, c), dtype=np.uint16)
    px[0] = (np.arange(w * c).reshape(w, c) * 257 % 65536).astype(np.uint16)
    if h > 2:
        px[2] = 0x8000 + (np.arange(w * c).reshape(w, c) % 256).astype(np.uint16)
    return px


def deep_files():
    """name -> (bytes, samples, bits): every 16-bit file of the decode tests"""
    files = {}
    for ctype, c in CHANNELS.items():
        for interlace in (False, True):
            for (w, h) in SIZES:
                px = picture16(ctype * 100 + w, w, h, c)
                files[f"ct{ctype}_{'a7' if interlace else 'ni'}_{w}x{h}.png"] = (write_png16(px, ctype, interlace), px, 16)
    for kind, c in ((5, 1), (6, 3)):
        for maxv in (65535, 1023):
            w, h = 7, 5
            v = np.random.default_rng(kind + maxv).integers(0, maxv + 1, (h, w, c)).astype(np.int64)
            v[0, 0], v[0, 1] = 0, maxv
            stored = v.copy()
            if maxv == 1023:
                stored[1, 0] = 2000                     # beyond maxval: clamped
                v[1, 0] = maxv
            want = ((v * 65535 + maxv // 2) // maxv).astype(np.uint16)
            data = f"P{kind}\n# deep\n{w} {h}\n{maxv}\n".encode() + stored.astype(">u2").tobytes()
            files[f"p{kind}_{maxv}.pnm"] = (data, want, 16 if maxv == 65535 else 10)
    for order in ("<", ">"):
        for c in (1, 3):
            w, h = 7, 5
            px = picture16(40 + c, w, h, c)
            files[f"{'le' if order == '<' else 'be'}{c}.tif"] = (write_tiff16(px, order), px, 16)
    return files


def write_tiff16(px, order):
    """A baseline TIFF, one uncompressed strip, 16 bits a sample, in either byte order"""
    h, w, c = px.shape
    strip = px.astype(order + "u2").tobytes()
    entries = [(256, 3, 1, w), (257, 3, 1, h), (258, 3, c, None), (259, 3, 1, 1), (262, 3, 1, 1 if c == 1 else 2), (273, 4, 1, None),
               (277, 3, 1, c), (278, 3, 1, h), (279, 4, 1, len(strip))]
    ifd_at = 8
    extra_at = ifd_at + 2 + 12 * len(entries) + 4
    bits = struct.pack(order + "H" * c, *([16] * c))
    strip_at = extra_at + (len(bits) if c > 1 else 0)
    out = (b"II*\x00" if order == "<" else b"MM\x00*") + struct.pack(order + "I", ifd_at) + struct.pack(order + "H", len(entries))
    for tag, typ, count, value in entries:
        if tag == 258:
            field = struct.pack(order + "I", extra_at) if c > 1 else struct.pack(order + "HH", 16, 0)
        elif tag == 273:
            field = struct.pack(order + "I", strip_at)
        else:
            field = struct.pack(order + "HH", value, 0) if typ == 3 else struct.pack(order + "I", value)
        out += struct.pack(order + "HHI", tag, typ, count) + field
    out += struct.pack(order + "I", 0) + (bits if c > 1 else b"") + strip
    return out


def test_16_bit_files_keep_both_bytes(codec, tmp_path):
    for name, (data, want, bits) in deep_files().items():
        p = tmp_path / name
        p.write_bytes(data)
        got = codec.decode16(p)
        assert got is not None, name
        assert got[0].shape == want.shape and got[1] == bits, (name, got[0].shape, got[1])
        assert (got[0] == want).all(), name
        high = codec.decode8(p)                    # the existing path is unchanged beside it
        assert high.shape[:2] == want.shape[:2]


def test_8_bit_files_come_back_promoted(codec, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(8)
    rgb = Image.fromarray(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8))
    rgba = Image.fromarray(rng.integers(0, 256, (9, 11, 4), dtype=np.uint8))
    cases = (("l.png", rgb.convert("L"), "PNG", {}, [0], 8), ("la.png", rgba.convert("LA"), "PNG", {}, [0, 3], 8),
             ("rgb.png", rgb, "PNG", {}, [0, 1, 2], 8), ("rgba.png", rgba, "PNG", {}, [0, 1, 2, 3], 8),
             ("rgb_a7.png", rgb, "PNG", {"interlace": 1}, [0, 1, 2], 8), ("pal.png", rgb.convert("P"), "PNG", {}, [0, 1, 2, 3], 8),
             ("bw.png", rgb.convert("1"), "PNG", {}, [0], 1), ("g4.png", rgb.convert("L").quantize(16), "PNG", {"bits": 4}, [0, 1, 2, 3], 4),
             ("q.jpg", rgb, "JPEG", {"quality": 90}, [0, 1, 2, 3], 8), ("b.bmp", rgb, "BMP", {}, [0, 1, 2, 3], 8),
             ("g.pgm", rgb.convert("L"), "PPM", {}, [0], 8), ("c.ppm", rgb, "PPM", {}, [0, 1, 2], 8),
             ("l.tif", rgb.convert("L"), "TIFF", {}, [0], 8), ("c.tif", rgb, "TIFF", {}, [0, 1, 2], 8))
    for name, im, fmt, kw, pick, bits in cases:
        p = tmp_path / name
        im.save(p, fmt, **kw)
        got = codec.decode16(p)
        assert got is not None, name
        want = codec.decode8(p)[:, :, pick].astype(np.uint16) * 257
        assert got[0].shape == want.shape and got[1] == bits, (name, got[0].shape, got[1])
        assert (got[0] == want).all(), name
    p = tmp_path / "p5_15.pgm"                   # a maxval of 8 bits or fewer: the 8-bit value times 257
    p.write_bytes(b"P5\n4 1\n15\n" + bytes([0, 1, 7, 15]))
    got = codec.decode16(p)
    assert got[1] == 4 and (got[0][0, :, 0] == codec.decode8(p)[0, :, 0].astype(np.uint16) * 257).all()
    assert codec.decode16(tmp_path / "missing.png") is None


def test_encoders(codec, tmp_path):
    from PIL import Image
    for (w, h) in SIZES + ((64, 40),):
        for c in (3, 1):
            px = picture16(w + c, w, h, c)
            if h > 4:
                px[3:] = (np.add.outer(np.arange(h - 3) * 300, np.arange(w) * 77)[:, :, None] + np.arange(c) * 1000).astype(np.uint16)  # smooth: every filter
            p = tmp_path / f"o{c}_{w}x{h}.png"
            assert codec.encode(p, px, png_only=True) == 0
            got, depth, ctype = read_png(p.read_bytes())
            assert depth == 16 and ctype == (0 if c == 1 else 2) and (got == px).all(), (w, h, c)
            back = codec.decode16(p)
            assert back[1] == 16 and (back[0] == px).all()
            if c == 1:
                im = Image.open(p)
                assert im.mode == "I;16" and (np.array(im) == px[:, :, 0]).all()
            q = tmp_path / f"o{c}_{w}x{h}.ppm"
            assert codec.encode(q, px) == 0
            data = q.read_bytes()
            head = f"P6\n{w} {h}\n65535\n".encode()
            assert data.startswith(head)
            samples = np.frombuffer(data[len(head):], ">u2").reshape(h, w, 3)
            assert (samples == (px if c == 3 else np.repeat(px, 3, axis=2))).all()
            assert (codec.decode16(q)[0] == samples).all()
    px = picture16(1, 4, 4, 3)
    assert codec.encode(tmp_path / "x.png", px) == 0 and codec.encode(tmp_path / "x.jpg", px) != 0 and codec.encode(tmp_path / "x.bmp", px) != 0
    assert codec.encode(tmp_path / "y.png", picture16(1, 4, 4, 2)) != 0 and codec.encode(tmp_path / "y.png", picture16(1, 4, 4, 4)) != 0


# ---- 3. the sanitizer program --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    from rusty_sr_amd.build import build_sanitized
    return build_sanitized()


def run_harness(harness, args, count):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1:max_allocation_size_mb=2048",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([harness, *map(str, args)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"sanitizer / crash (rc {r.returncode}):\n{r.stderr[-3000:]}"
    lines = r.stdout.strip().splitlines()
    assert len(lines) == count and all(l.startswith("ok ") or l.startswith("error: ") for l in lines), lines[:5]
    return lines


def test_mangled_16_bit_files_fail_cleanly(harness, tmp_path):
    """Every truncation point of every file (the 1x1, 5x7 and 33x17 PNGs of every colour type, non-interlaced and Adam7, the PNM and
    TIFF files) and seeded bit flips of all of them, through the deep decode path under AddressSanitizer + UBSan."""
    files = deep_files()
    rng = np.random.default_rng(16)
    paths, intact = [], []
    for name, (data, _, _) in files.items():
        stem, ext = os.path.splitext(name)
        p = tmp_path / name
        p.write_bytes(data)
        intact.append(p)
        for c in range(len(data)):
            q = tmp_path / f"{stem}_cut{c}{ext}"
            q.write_bytes(data[:c])
            paths.append(q)
        for k in range(30):
            b = bytearray(data)
            for _ in range(int(rng.integers(1, 4))):
                pos = int(rng.integers(0, min(len(b), 120))) if k % 2 == 0 else int(rng.integers(0, len(b)))
                b[pos] ^= 1 << int(rng.integers(0, 8))
            q = tmp_path / f"{stem}_flip{k}{ext}"
            q.write_bytes(bytes(b))
            paths.append(q)
    lines = run_harness(harness, ["--u16", *intact], len(intact))
    assert all(l.startswith("ok ") for l in lines), lines
    assert len(paths) == sum(len(d) + 30 for d, _, _ in files.values()) and len(paths) > 25000
    for i in range(0, len(paths), 400):
        run_harness(harness, ["--u16", *paths[i:i + 400]], len(paths[i:i + 400]))


def test_16_bit_round_trip_under_sanitizers(harness, tmp_path):
    for c in (1, 3):
        for (w, h) in ((1, 1), (33, 17), (640, 360)):
            assert run_harness(harness, ["--roundtrip16", w, h, c, tmp_path / f"rt{c}.png"], 1) == [f"ok {w}x{h} {c}"]


# ---- 4. the ABI in its four places ---------------------------------------------------------------------------------------------------
def test_the_eight_names_in_all_four_places():
    from rusty_sr_amd._lib import SYMBOLS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srhip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust_host", "src", "srhip.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, arity in zip(NAMES, ARITY):
        assert name in SYMBOLS and len(SYMBOLS[name][1]) == arity and SYMBOLS[name][0] is C.c_int, name
        m = re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m and len(m.group(1).split(",")) == arity, name
        for text in (rust, doc):
            m = re.search(r"pub fn %s\(([^)]*)\)\s*->\s*c_int;" % name, text)
            assert m and len(m.group(1).split(",")) == arity, name
    assert "Deep colour" in header or "Deep colour" in open(os.path.join(ROOT, "include", "srhip.h")).read()
    assert "--depth" in doc


# ---- 5. the CLI's refusals -----------------------------------------------------------------------------------------------------------
def test_cli_refusals_name_the_argument_and_touch_no_device(tmp_path):
    from rusty_sr_amd.build import build_host
    build_host()
    src = tmp_path / "in.png"
    src.write_bytes(write_png16(picture16(1, 5, 7, 3), 2))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")      # no device present: a call that reached one would not exit 2

    def run(*args):
        return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60, env=env)

    for args, words in ((("--depth", "16", "--alpha", str(src), str(tmp_path / "o.png")), ("--depth 16", "--alpha")),
                        (("--depth", "16", "--devices", "0,1", str(src), str(tmp_path / "o.png")), ("--depth 16", "more than one device")),
                        (("--depth", "16", str(src), str(tmp_path / "o.jpg")), ("--depth 16", ".jpg")),
                        (("--depth", "16", str(src), str(tmp_path / "o.JPEG")), ("--depth 16", ".jpeg")),
                        (("--depth=16", str(src), str(tmp_path / "o.bmp")), ("--depth 16", ".bmp")),
                        (("--depth", "12", str(src), str(tmp_path / "o.png")), ("'12'", "--depth <BITS>", "8", "16", "auto")),
                        (("--depth=", str(src), str(tmp_path / "o.png")), ("--depth <BITS>",)),
                        (("--depth",), ("--depth <BITS>", "requires a value"))):
        res = run(*args)
        assert res.returncode == 2, (args, res.returncode, res.stderr)
        for word in words:
            assert word in res.stderr, (args, word, res.stderr)
        assert not list(tmp_path.glob("o.*"))
    res = run("--help")
    assert res.returncode == 0 and "--depth <BITS>" in res.stdout and "[values: 8, 16, auto]" in res.stdout
