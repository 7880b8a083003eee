"""The fixture cases of the degradation operator's tests: tests/test_gpu_degrade.py runs every one of them on the device and demands the
reference's bytes; tests/test_degrade_cpu.py checks on the reference alone that no value of any of them sits within 1e-11 of a rounding
boundary -- the condition that makes that demand fair.  If a case fails it, change its seed, not the bound."""
import numpy as np

from conftest import synth_u8

ALL = dict(sigma=1.7, noise=25.0, quality=50)


def image(kind, seed, h, w, ch=3):
    if kind == "black":
        return np.zeros((h, w, ch), np.uint8)
    if kind == "white":
        return np.full((h, w, ch), 255, np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)
    px = synth_u8(seed, 1, h, w)[0]  # smooth: what a photograph's crop looks like
    if ch == 4:
        px = np.concatenate([px, np.random.default_rng(seed + 1).integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    return px


def _case(name, img, factor, window, member=0, sigma=0.0, noise=0.0, quality=0, seed=0):
    return dict(name=name, img=img, factor=factor, window=window, member=member, sigma=sigma, noise=noise, quality=quality, seed=seed)


def cases():
    """-> a list of dicts: name, img = (kind, seed, h, w, ch), factor, window = (y0, x0, frame_h, frame_w), member, sigma, noise, quality, seed."""
    out = []
    n = 0
    # every factor x LR size (one block; ragged blocks; several blocks), every stage on, the window inside a larger image
    for f in (2, 3, 4):
        for lh, lw in ((8, 8), (13, 10), (16, 24)):
            n += 1
            out.append(_case(f"all-f{f}-{lh}x{lw}", ("smooth", n, f * lh + 9, f * lw + 11, 3), f, (4, 5, f * lh, f * lw), seed=1000 + n, **ALL))
    # each stage alone, and none (radius 1, 6, 12; quality at both ends of the scale rule)
    img = ("smooth", 21, 48, 41, 3)
    win = (5, 6, 39, 30)
    out.append(_case("none", img, 3, win))
    for s in (0.3, 1.7, 4.0):
        out.append(_case(f"blur-{s}", img, 3, win, sigma=s))
    out.append(_case("noise-25", img, 3, win, noise=25.0, seed=77))
    for q in (1, 50, 100):
        out.append(_case(f"jpeg-{q}", img, 3, win, quality=q))
    # a blur radius (12) larger than the whole image
    out.append(_case("blur-4-tiny-image", ("smooth", 22, 13, 10, 3), 2, (0, 0, 12, 10), sigma=4.0, quality=75))
    # the 8 members on a frame that is not square (the source window of k >= 4 is 20 x 26)
    for k in range(8):
        out.append(_case(f"member-{k}", ("smooth", 30, 40, 37, 3), 2, (3, 6, 26, 20), member=k, seed=2000 + k, **ALL))
    # windows that overhang each edge, and windows wholly outside the image
    for name, y0, x0 in (("top", -7, 2), ("left", 3, -9), ("bottom", 15, 2), ("right", 3, 14), ("outside-before", -100, -100),
                         ("outside-after", 40, 40)):
        out.append(_case(f"window-{name}", ("smooth", 31, 30, 28, 3), 3, (y0, x0, 24, 24), seed=3000 + len(out), **ALL))
    out.append(_case("window-corner-member-5", ("smooth", 32, 30, 28, 3), 3, (-5, 20, 24, 18), member=5, seed=3100, **ALL))
    # RGBA sources: alpha is dropped
    out.append(_case("rgba-f4", ("smooth", 40, 45, 47, 4), 4, (6, 7, 32, 32), seed=4000, **ALL))
    out.append(_case("rgba-f3-ragged", ("smooth", 41, 50, 44, 4), 3, (2, 3, 39, 30), member=3, seed=4001, **ALL))
    # clamps on both sides: black and white under noise, random noise at both ends of the quality scale
    out.append(_case("black", ("black", 0, 30, 30, 3), 3, (0, 0, 30, 30), noise=25.0, quality=50, seed=5000))
    out.append(_case("white", ("white", 0, 30, 30, 3), 3, (0, 0, 30, 30), noise=25.0, quality=50, seed=5001))
    out.append(_case("noise-image-q1", ("noise", 50, 34, 36, 3), 2, (1, 2, 32, 32), quality=1))
    out.append(_case("noise-image-q100", ("noise", 51, 34, 36, 3), 2, (1, 2, 32, 32), sigma=0.3, noise=64.0, quality=100, seed=5003))
    # the dearest setting: factor 4, radius 12, several blocks
    out.append(_case("dearest", ("smooth", 60, 80, 110, 3), 4, (8, 7, 64, 96), sigma=4.0, noise=8.0, quality=60, seed=6000))
    return out


def params(case):
    """The keyword arguments of degrade_ref.degrade / Engine.degrade for a case."""
    return {k: case[k] for k in ("sigma", "noise", "quality", "seed", "window", "member")}
