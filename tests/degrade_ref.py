"""The degradation operator of include/srhip.h ("Degradation") restated in numpy: blur, pool, noise and a JPEG round trip of a window of an
HR image, in f64.  No GPU is needed; tests/test_degrade_cpu.py holds this restatement to its own rounding rule, to the oracle's pool and to
Pillow, and tests/test_gpu_degrade.py holds the kernels to it byte for byte.

`degrade(...)` takes an arithmetic: `F64` (numpy float64, sums in the order the header gives), `LONGDOUBLE` (the same in numpy longdouble)
or `REASSOCIATED` (float64, every sum taken in the opposite order).  The bytes must not depend on it (the rounding rule's bias, 2^-30, is
what makes that so); `trace=` collects, per rounding site, the distance of every value from its rounding boundary."""
import math
import re

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
BIAS = 2.0 ** -30
MAX_SIGMA, MAX_NOISE = 4.0, 64.0

# ITU-T T.81 Annex K, tables K.1 and K.2, in natural (row-major) order: row = vertical frequency
LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


class Arith:
    def __init__(self, name, dtype, reverse):
        self.name, self.dtype, self.reverse = name, dtype, reverse

    def sum(self, terms):
        """The sum of a list of arrays (or scalars) in list order -- or in the opposite order."""
        terms = list(terms)
        if self.reverse:
            terms = terms[::-1]
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        return acc


F64 = Arith("f64", np.float64, False)
LONGDOUBLE = Arith("longdouble", np.longdouble, False)
REASSOCIATED = Arith("reassociated", np.float64, True)


def mix(z):
    """SplitMix64's output function of the state z (a Python int)."""
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def stream_output(seed, j):
    """Output number j (1, 2, ...) of the SplitMix64 stream seeded with `seed`: random access."""
    return mix(seed + j * GOLDEN)


def uniform(x):
    return (x >> 11) * 2.0 ** -53


def srgb_to_linear_table():
    """SrgbToLinear(byte / 255) for the 256 bytes, f64, by the C library's pow (what the library's host side builds)."""
    out = []
    for b in range(256):
        s = b / 255.0
        out.append(s / 12.92 if s <= 0.04045 else math.pow((s + 0.055) / 1.055, 2.4))
    return np.array(out, np.float64)


def linear_to_srgb(l):
    l = np.asarray(l)
    hi = np.asarray(1.055, l.dtype) * np.power(np.maximum(l, 0), np.asarray(1.0, l.dtype) / np.asarray(2.4, l.dtype)) - np.asarray(0.055, l.dtype)
    return np.where(l <= 0.0031308, np.asarray(12.92, l.dtype) * l, hi)


def dct_matrix():
    """C[u][x] = cos((2x + 1) u pi / 16) / 2, row 0 divided by sqrt 2."""
    c = [[0.5 * math.cos((2 * x + 1) * u * math.pi / 16.0) for x in range(8)] for u in range(8)]
    c[0] = [v / math.sqrt(2.0) for v in c[0]]
    return np.array(c, np.float64)


def quant_table(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.array([min(max((b * scale + 50) // 100, 1), 255) for b in base], np.float64).reshape(8, 8)


def _note(trace, site, v):
    """Record |frac(|v| + 0.5 + 2^-30)| distances: how far each value is from the point where its rounding changes."""
    if trace is None:
        return
    a = np.abs(np.asarray(v, np.float64)) + 0.5 + BIAS
    fr = a - np.floor(a)
    trace.setdefault(site, []).append(np.minimum(fr, 1.0 - fr).ravel())


def rnd(v, trace=None, site=""):
    """R(v) = sign(v) floor(|v| + 0.5 + 2^-30); for v >= 0 that is floor(v + 0.5 + 2^-30)."""
    _note(trace, site, v)
    v = np.asarray(v)
    return (np.sign(v) * np.floor(np.abs(v) + np.asarray(0.5 + BIAS, v.dtype))).astype(np.float64)


def source_plane(hr):
    """S(y, x): a function of integer index ARRAYS -> (..., 3) u8: the image's RGB inside the image, 0 outside."""
    hr = np.asarray(hr)
    h, w = hr.shape[:2]

    def S(y, x):
        inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        px = hr[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1), :3]
        return np.where(inside[..., None], px, 0).astype(np.uint8)

    return S


def frame_pixels(hr, y0, x0, win_h, win_w, k, p, q):
    """Batch-frame pixels (p, q) (integer arrays, ANY values) of member k of the window: the crop kernels' mapping (the frame is win_h x
    win_w; the source window at (y0, x0) is win_w x win_h, rows x columns, when k & 4), without bounds on p and q."""
    if k & 2:
        p = win_h - 1 - p
    if k & 1:
        q = win_w - 1 - q
    sy, sx = (y0 + q, x0 + p) if k & 4 else (y0 + p, x0 + q)
    return source_plane(hr)(sy, sx)


def blur_weights(sigma, ar=F64):
    """sigma as the f32 the struct carries.  -> (radius, weights[2 radius + 1]) normalised, the sum taken in tap order."""
    s = float(np.float32(sigma))
    if not s > 0:
        return 0, np.ones(1, ar.dtype)
    r = int(math.ceil(3.0 * s))
    d = np.arange(-r, r + 1).astype(np.float64)
    w = np.array([math.exp(-(t * t) / (2.0 * s * s)) for t in d], np.float64).astype(ar.dtype)
    return r, w / ar.sum(list(w))


def jpeg_round_trip(b, quality, ar=F64, trace=None):
    """b: (lh, lw, 3) integer-valued f64 in [0, 255] -> the same after a 4:4:4 JPEG round trip of that quality (no entropy coding: it is
    lossless).  Blocks are anchored at (0, 0); ragged edges replicate the last row / column."""
    lh, lw = b.shape[:2]
    ph, pw = -(-lh // 8) * 8, -(-lw // 8) * 8
    pad = b[np.minimum(np.arange(ph), lh - 1)][:, np.minimum(np.arange(pw), lw - 1)].astype(ar.dtype)
    R, G, B = pad[..., 0], pad[..., 1], pad[..., 2]
    k = lambda v: np.asarray(v, ar.dtype)
    ycc = [ar.sum([k(0.299) * R, k(0.587) * G, k(0.114) * B]),
           ar.sum([k(128.0) - k(0.168735892) * R, -(k(0.331264108) * G), k(0.5) * B]),
           ar.sum([k(128.0) + k(0.5) * R, -(k(0.418687589) * G), -(k(0.081312411) * B)])]
    Cm = dct_matrix().astype(ar.dtype)
    planes = []
    for ci, plane in enumerate(ycc):
        plane = np.clip(rnd(plane, trace, "ycc"), 0, 255).astype(ar.dtype) - k(128.0)
        t = quant_table(LUMA if ci == 0 else CHROMA, quality).astype(ar.dtype)
        blk = plane.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3)          # (by, bx, y, x)
        tmp = ar.sum([Cm[:, y][None, None, :, None] * blk[:, :, y, None, :] for y in range(8)])      # (by, bx, u, x) = sum_y C[u][y] b[y][x]
        coef = ar.sum([tmp[:, :, :, x, None] * Cm[:, x][None, None, None, :] for x in range(8)])     # (by, bx, u, v) = sum_x tmp[u][x] C[v][x]
        qz = rnd(coef / t, trace, "quant").astype(ar.dtype) * t
        tmp = ar.sum([Cm[u, :][None, None, :, None] * qz[:, :, u, None, :] for u in range(8)])       # (by, bx, y, v) = sum_u C[u][y] d[u][v]
        out = ar.sum([tmp[:, :, :, v, None] * Cm[v, :][None, None, None, :] for v in range(8)])      # (by, bx, y, x) = sum_v tmp[y][v] C[v][x]
        out = np.clip(rnd(out + k(128.0), trace, "idct"), 0, 255).astype(ar.dtype)
        planes.append(out.transpose(0, 2, 1, 3).reshape(ph, pw))
    Y, Cb, Cr = planes[0], planes[1] - k(128.0), planes[2] - k(128.0)
    rgb = [ar.sum([Y, k(1.402) * Cr]),
           ar.sum([Y, -(k(0.344136286) * Cb), -(k(0.714136286) * Cr)]),
           ar.sum([Y, k(1.772) * Cb])]
    out = np.stack([np.clip(rnd(c, trace, "rgb"), 0, 255) for c in rgb], axis=-1)
    return out[:lh, :lw]


def noise_values(noise, seed, count):
    """noise sqrt(-2 ln(1 - u1)) cos(2 pi u2) for value indices 0 .. count-1 (f64; noise as the f32 the struct carries)."""
    n = float(np.float32(noise))
    out = np.empty(count, np.float64)
    for i in range(count):
        u1, u2 = uniform(stream_output(seed, 2 * i + 1)), uniform(stream_output(seed, 2 * i + 2))
        out[i] = n * math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(2.0 * math.pi * u2)
    return out


def degrade(hr, factor, sigma=0.0, noise=0.0, quality=0, seed=0, window=None, member=0, ar=F64, trace=None):
    """hr: (h, w, 3|4) u8.  window: (y0, x0, win_h, win_w) in HR pixels, the batch frame's size (default: the image cropped to a multiple of
    the factor, at the origin).  -> (win_h / f, win_w / f, 3) u8."""
    hr = np.asarray(hr)
    f = int(factor)
    if window is None:
        window = (0, 0, hr.shape[0] // f * f, hr.shape[1] // f * f)
    y0, x0, win_h, win_w = (int(v) for v in window)
    if not 2 <= f <= 4 or win_h < f or win_w < f or win_h % f or win_w % f or not 0 <= member <= 7:
        raise ValueError("invalid geometry")
    if not (0 <= float(np.float32(sigma)) <= MAX_SIGMA and 0 <= float(np.float32(noise)) <= MAX_NOISE and 0 <= quality <= 100):
        raise ValueError("invalid parameters")
    lh, lw = win_h // f, win_w // f
    r, wts = blur_weights(sigma, ar)
    tab = srgb_to_linear_table().astype(ar.dtype)
    p, q = np.meshgrid(np.arange(-r, win_h + r), np.arange(-r, win_w + r), indexing="ij")
    lin = tab[frame_pixels(hr, y0, x0, win_h, win_w, member, p, q)]                         # (win_h + 2r, win_w + 2r, 3)
    if r:
        lin = ar.sum([wts[t] * lin[:, t:t + win_w] for t in range(2 * r + 1)])            # rows: along q
        lin = ar.sum([wts[t] * lin[t:t + win_h] for t in range(2 * r + 1)])               # then columns: along p
    blocks = lin.reshape(lh, f, lw, f, 3)
    mean = ar.sum([blocks[:, i, :, j] for i in range(f) for j in range(f)]) / np.asarray(f * f, ar.dtype)
    v = np.asarray(255.0, ar.dtype) * linear_to_srgb(mean)
    if float(np.float32(noise)) > 0:
        v = v + noise_values(noise, seed, lh * lw * 3).reshape(lh, lw, 3).astype(ar.dtype)
    b = np.clip(rnd(v, trace, "pixel"), 0, 255)
    if quality:
        b = jpeg_round_trip(b, quality, ar, trace)
    return b.astype(np.uint8)


# ---- the CLI's --degrade SPEC and its draws (rusty_sr_amd.degrade_spec is the product's twin of this rule)

SPEC_KEYS = {"blur": (0.0, MAX_SIGMA, False), "noise": (0.0, MAX_NOISE, False), "jpeg": (0, 100, True)}


def parse_spec(text):
    """'blur=A[:B],noise=A[:B],jpeg=A[:B]' -> {key: (A, B)}; keys that are absent are (0, 0).  ValueError names the key."""
    out = {k: (0, 0) if integer else (0.0, 0.0) for k, (_, _, integer) in SPEC_KEYS.items()}
    seen = set()
    if not text:
        raise ValueError("empty degrade spec")
    for part in text.split(","):
        key, eq, val = part.partition("=")
        if key not in SPEC_KEYS:
            raise ValueError(f"unknown key '{key}'")
        if not eq or key in seen:
            raise ValueError(f"malformed or repeated key '{key}'")
        seen.add(key)
        lo, hi, integer = SPEC_KEYS[key]
        try:
            if not all(re.fullmatch(r"[+-]?\d+" if integer else r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", v) for v in val.split(":")):
                raise ValueError(val)
            ab = [int(v) if integer else float(v) for v in val.split(":")]
        except ValueError:
            raise ValueError(f"malformed value for '{key}'") from None
        if len(ab) not in (1, 2) or any(not math.isfinite(v) for v in ab):
            raise ValueError(f"malformed value for '{key}'")
        a, b = ab[0], ab[-1]
        if b < a:
            raise ValueError(f"reversed range for '{key}'")
        if a < lo or b > hi:
            raise ValueError(f"range for '{key}' outside {lo}..{hi}")
        out[key] = (a, b)
    return out


def draws(spec, seed, count):
    """The first `count` draws of a spec under `seed`: dicts of sigma, noise, quality, seed (four stream outputs per draw)."""
    s = (seed ^ 0xD6E8FEB86659FD93) & MASK
    out = []
    for i in range(count):
        x = [stream_output(s, 4 * i + j) for j in (1, 2, 3, 4)]
        (a0, b0), (a1, b1), (a2, b2) = spec["blur"], spec["noise"], spec["jpeg"]
        out.append({"sigma": a0 + uniform(x[0]) * (b0 - a0), "noise": a1 + uniform(x[1]) * (b1 - a1),
                    "quality": a2 + int(math.floor(uniform(x[2]) * (b2 - a2 + 1))), "seed": x[3]})
    return out
