"""The resampling rule of include/srhip.h ("Resampling to any size"), restated in numpy, f64 throughout: a separable resampler in Pillow's
convention (tests/test_resize_cpu.py holds it to Pillow's mode-F Image.resize).  Not used by the product."""
import numpy as np

FILTERS = ("box", "triangle", "catrom", "lanczos3")
SUPPORT = {"box": 0.5, "triangle": 1.0, "catrom": 2.0, "lanczos3": 3.0}


def filter_value(name, x):
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    if name == "box":
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    if name == "triangle":
        return np.maximum(0.0, 1.0 - a)
    if name == "catrom":  # Keys, a = -0.5
        return np.where(a < 1.0, (1.5 * a - 2.5) * a * a + 1.0, np.where(a < 2.0, ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0, 0.0))
    if name == "lanczos3":
        return np.where(a < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)
    raise ValueError(name)


def taps(n_in, n_out, name):
    """[(lo, weights)] for the n_out output indices of an axis: taps lo .. lo + len(weights) - 1, weights normalised to 1."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    s = SUPPORT[name] * fs
    out = []
    for o in range(n_out):
        c = (o + 0.5) * scale
        lo = max(int(np.trunc(c - s + 0.5)), 0)
        hi = min(int(np.trunc(c + s + 0.5)), n_in)
        w = filter_value(name, (np.arange(lo, hi) + 0.5 - c) / fs)
        out.append((lo, w / w.sum()))
    return out


def resize_axis(x, axis, n_out, name):
    """x resampled along `axis` to n_out samples, taps summed in ascending index."""
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    out = np.zeros((n_out,) + x.shape[1:], dtype=np.float64)
    for o, (lo, w) in enumerate(taps(x.shape[0], n_out, name)):
        for k, wk in enumerate(w):
            out[o] += wk * x[lo + k]
    return np.moveaxis(out, 0, axis)


def srgb_to_linear(s):
    s = np.asarray(s, dtype=np.float64)
    return np.where(s <= 0.04045, s / 12.92, np.power((np.maximum(s, 0.04045) + 0.055) / 1.055, 2.4))


def linear_to_srgb(l):
    l = np.asarray(l, dtype=np.float64)
    return np.where(l <= 0.0031308, 12.92 * l, 1.055 * np.power(np.maximum(l, 0.0031308), 1.0 / 2.4) - 0.055)


def resize_plane(x, size, name):
    """(.., h, w) -> (.., oh, ow): columns first, then rows, no transfer function (what Pillow's mode F computes)."""
    oh, ow = size
    return resize_axis(resize_axis(x, -1, ow, name), -2, oh, name)


def resize(x, size, name="lanczos3", srgb_space=False):
    """(.., h, w, 3) sRGB values (u8 pixels: byte / 255, alpha dropped) -> (.., oh, ow, 3) f64, pre-quantisation."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        x = x[..., :3].astype(np.float64) / 255.0
    x = x.astype(np.float64)
    oh, ow = size
    if not srgb_space:
        x = srgb_to_linear(x)
    y = resize_axis(resize_axis(x, -2, ow, name), -3, oh, name)
    return y if srgb_space else linear_to_srgb(y)


def quantise(v):
    """data_to_img: clamp(floor(255 v + 0.5)), alpha 255 -> (.., 4) u8."""
    q = np.clip(np.floor(255.0 * np.asarray(v, dtype=np.float64) + 0.5), 0, 255).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def scaled_size(h, w, s):
    """--scale S of the CLI: max(1, floor(in S + 0.5)) per axis -> (oh, ow)."""
    return max(1, int(np.floor(h * s + 0.5))), max(1, int(np.floor(w * s + 0.5)))
