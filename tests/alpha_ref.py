"""The transparency rules of include/srhip.h ("Transparency") restated in numpy, in the integers the header gives: the GPU kernels must
agree bit for bit.  Nothing here is derived from the code under test."""
import numpy as np


def bleed(px, radius):
    """(h, w, 4) or (n, h, w, 4) u8 -> the same shape: R Jacobi steps of the 8-neighbour mean of the known colours, rounded half up."""
    px = np.asarray(px, dtype=np.uint8)
    if px.ndim == 4:
        return np.stack([bleed(p, radius) for p in px])
    h, w, _ = px.shape
    c = px[..., :3].astype(np.int64)
    known = px[..., 3] > 0
    for _ in range(int(radius)):
        if known.all() or not known.any():
            break
        kp = np.zeros((h + 2, w + 2), dtype=np.int64)
        kp[1:-1, 1:-1] = known
        cp = np.zeros((h + 2, w + 2, 3), dtype=np.int64)
        cp[1:-1, 1:-1] = c * known[..., None]
        cnt = np.zeros((h, w), dtype=np.int64)
        tot = np.zeros((h, w, 3), dtype=np.int64)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if dy == 1 and dx == 1:
                    continue
                cnt += kp[dy:dy + h, dx:dx + w]
                tot += cp[dy:dy + h, dx:dx + w]
        fill = ~known & (cnt > 0)
        n = np.maximum(cnt, 1)[..., None]
        c = np.where(fill[..., None], (2 * tot + n) // (2 * n), c)
        known = known | fill
    out = px.copy()
    out[..., :3] = c.astype(np.uint8)
    return out


def axis_taps(length, f):
    """Per output index of an axis: the two clamped tap indices and their weights out of 2 f."""
    o = np.arange(length * f)
    i, m = o // f, 2 * (o % f) + 1 - f
    t0 = np.where(m >= 0, i, i - 1)
    w0 = np.where(m >= 0, 2 * f - m, -m)
    w1 = 2 * f - w0
    return np.clip(t0, 0, length - 1), np.clip(t0 + 1, 0, length - 1), w0, w1


def up_alpha_sum(a, f):
    """(h, w) alpha -> (f h, f w) int64 S = sum wy wx a, the exact bilinear value times 4 f^2."""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    y0, y1, wy0, wy1 = axis_taps(h, f)
    x0, x1, wx0, wx1 = axis_taps(w, f)
    rows = a[y0] * wy0[:, None] + a[y1] * wy1[:, None]
    return rows[:, x0] * wx0[None, :] + rows[:, x1] * wx1[None, :]


def up_alpha(a, f):
    """(h, w) or (n, h, w) u8 alpha -> (.., f h, f w) u8: (S + 2 f^2) div (4 f^2)."""
    a = np.asarray(a, dtype=np.uint8)
    if a.ndim == 3:
        return np.stack([up_alpha(x, f) for x in a])
    return ((up_alpha_sum(a, f) + 2 * f * f) // (4 * f * f)).astype(np.uint8)


def transform(x, k):
    """T_k of the self-ensemble on an (h, w, C) image: swap the spatial axes if k & 4, then reverse the rows if k & 2, the columns if k & 1."""
    if k & 4:
        x = x.transpose(1, 0, 2)
    if k & 2:
        x = x[::-1]
    if k & 1:
        x = x[:, ::-1]
    return np.ascontiguousarray(x)


def disc_sprite(colour=(200, 120, 40), size=40, radius=10):
    """The constant sprite: a disc of one colour at alpha 255 in the middle of a size x size image, black at alpha 0 elsewhere.  Returns
    the image and the Chebyshev distance of every pixel to the disc."""
    yy, xx = np.mgrid[0:size, 0:size]
    cy = cx = size // 2
    inside = (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius
    px = np.zeros((size, size, 4), dtype=np.uint8)
    px[inside, :3] = colour
    px[inside, 3] = 255
    ys, xs = np.nonzero(inside)
    dist = np.min(np.maximum(np.abs(yy[..., None] - ys), np.abs(xx[..., None] - xs)), axis=-1)
    return px, dist


def hole_radius(radius):
    """The Euclidean radius rho of the "hole" pattern: a visible pixel lies more than rho from the centre, so one of its two offsets is
    more than rho / sqrt(2) >= 1.06 (R + 1): the centre is farther than R (Chebyshev) from every visible pixel and stays unfilled."""
    return (3 * (radius + 1) + 1) // 2


def alpha_pattern(name, h, w, radius, seed=0):
    """The alpha patterns of the bleed tests over random colours (also under alpha 0: the bleed must overwrite, or keep, real values)."""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a = rng.integers(1, 256, (h, w), dtype=np.uint8)
    if name == "sparse":
        a[rng.random((h, w)) >= 0.1] = 0
    elif name == "dense":
        a[rng.random((h, w)) < 0.5] = 0
    elif name == "opaque":
        pass
    elif name == "transparent":
        a[:] = 0
    elif name == "corner":
        a[:] = 0
        a[-1, -1] = 7
    elif name == "hole":  # a transparent disc whose middle the bleed cannot reach, where the image has room for it
        yy, xx = np.mgrid[0:h, 0:w]
        a[(yy - h // 2) ** 2 + (xx - w // 2) ** 2 <= hole_radius(radius) ** 2] = 0
    else:
        raise ValueError(name)
    px[..., 3] = a
    return px
