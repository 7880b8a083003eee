"""HR images in the pixel ranges that conftest.synth_u8 (bytes 37 .. 215) and rng.random never reach -- dark, bright, constant, every
byte value, out of [0, 1], and the floats around the sRGB threshold -- and the tables of cases built on them.  Every sRGB transfer
function of the training graph (rusty_sr_amd/csrc/sr_transfer.h, the byte table of sr_valid.cpp, SrgbToLinear' of sr_grad.hip) has a
linear and a power branch; these classes are what takes the linear one, and the power one beyond 1.

No GPU here: tests/test_pixel_classes_cpu.py proves on the f64 restatement alone that each case reaches the branch it is meant for
and is well enough conditioned for the bar it is held to, and tests/test_gpu_pixel_ranges.py runs the same tables on the GPU."""
import numpy as np

F32_THRESH = np.float32(0.04045)   # SrgbToLinear's branch point as the devices compare it
LIN_THRESH = 0.0031308             # LinearToSrgb's

U8_CLASSES = ("dark_u8", "bright_u8", "noise_u8", "black", "white", "ramp_u8")
F32_CLASSES = ("dark_f32", "wide_f32", "edge_f32", "far_f32")
CLASSES = U8_CLASSES + F32_CLASSES
UNIT_CLASSES = tuple(c for c in CLASSES if c != "far_f32")   # within [-0.5, 1.5]: the pool's absolute bar holds


def edge_values():
    """float32(0.04045), the 32 representable values on either side of it, and exact 0.0, 1.0, -0.0"""
    bits = F32_THRESH.view(np.uint32).astype(np.int64) + np.arange(-32, 33)
    return bits.astype(np.uint32).view(np.float32), np.array([0.0, 1.0, -0.0], dtype=np.float32)


def ramp_u8(n, h, w):
    """Byte (t + 85 c) % 256 in channel c of pixel (y, x), t = x // 4 + y * (w // 4): wherever h * (w // 4) >= 256 every byte value
    stands in every channel at every x % 4 -- of an RGB row, at every byte position mod 4."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    img = ((x // 4 + y * max(w // 4, 1) + 85 * c) % 256).astype(np.uint8)
    return np.stack([np.roll(img, 7 * i, axis=0) for i in range(n)])


def make(cls, seed, n, h, w, ch=3):
    """-> (n, h, w, ch) u8 for the *_u8 classes and the constants (ch 3 or 4: a random alpha, which every pass must ignore), else
    (n, h, w, 3) f32."""
    rng = np.random.default_rng(seed)
    shape = (n, h, w, 3)
    if cls in U8_CLASSES:
        if cls == "dark_u8":
            px = rng.integers(0, 24, shape, dtype=np.uint8)
        elif cls == "bright_u8":
            px = rng.integers(232, 256, shape, dtype=np.uint8)
        elif cls == "noise_u8":
            px = rng.integers(0, 256, shape, dtype=np.uint8)
        elif cls == "black":
            px = np.zeros(shape, np.uint8)
        elif cls == "white":
            px = np.full(shape, 255, np.uint8)
        else:
            px = ramp_u8(n, h, w)
        if ch == 4:
            px = np.concatenate([px, rng.integers(0, 256, (n, h, w, 1), dtype=np.uint8)], axis=-1)
        return np.ascontiguousarray(px)
    assert ch == 3, "an f32 image has 3 channels"
    if cls == "dark_f32":
        return rng.uniform(-0.02, 0.09, shape).astype(np.float32)
    if cls == "wide_f32":
        return rng.uniform(-0.5, 1.5, shape).astype(np.float32)
    if cls == "far_f32":
        return rng.uniform(-8, 50, shape).astype(np.float32)
    if cls == "edge_f32":
        near, exact = edge_values()
        px = near[rng.integers(0, near.size, shape)]
        pick = rng.random(shape)
        for k, v in enumerate(exact):   # a tenth of the values each
            px = np.where((pick >= 0.1 * k) & (pick < 0.1 * (k + 1)), v, px)
        return np.ascontiguousarray(px.astype(np.float32))
    raise ValueError(cls)


def is_u8(cls):
    return cls in U8_CLASSES


def image_seed(cls, f, h, w):
    return 1000 * CLASSES.index(cls) + 100 * f + 7 * h + w


# ---- pool and forward loss -----------------------------------------------------------------------------------------------------------
def pool_shapes(f):
    """one LR pixel; several, not a multiple of f; more than one workgroup of the pool.  Widths of the crop (7 f, 30 f): not a
    multiple of 4 at f = 2 (14) and f = 3 (21, 90)."""
    return [(f, f), (5 * f + 1, 7 * f + 2), (24 * f, 30 * f + 1)]


def channels_of(cls, f, k=0):
    """3 or 4 channels for a u8 class, so that both appear for every class over the factors and shapes"""
    return 3 + (CLASSES.index(cls) + f + k) % 2 if is_u8(cls) else 3


def synthetic_weights(f):
    from test_grad_restatement import synthetic_params
    return synthetic_params(f, 100 + f)


def weights_of(key, f, params):
    """key "synthetic": seeded weights at the bundled weights' scales; else a bundled set (factor 3), from the `params` fixture"""
    if key == "synthetic":
        return synthetic_weights(f)
    assert f == 3
    return params[key]


# ---- gradient cases: (class, factor, n, h, w, channels, linear_loss, weights) ------------------------------------------------------------
# Synthetic weights throughout: with the bundled, trained weights the residual on constant and near-constant images (black, white,
# bright_u8) is ~0.02, so that the f32 rounding of the output is a visible fraction of it -- the f32 run of the restatement itself is
# then 1.5e-5 .. 4e-5 from the f64 one, and the 1e-4 bar of assert_grad_close would measure the conditioning of the case, not the kernel.
# imagenet is kept for the two classes where it is well conditioned.  test_pixel_classes_cpu.py gates every row at 1e-5.
GRAD_CLASSES = ("dark_u8", "bright_u8", "noise_u8", "black", "white", "ramp_u8", "dark_f32", "wide_f32", "edge_f32")
DARK_GRAD_CLASSES = ("dark_u8", "black", "dark_f32")     # shares of the restatement's outputs <= 0.04045 and < 0
BRIGHT_GRAD_CLASSES = ("bright_u8", "white")             # ... and > 1


def _grad_cases():
    out = []
    for i, cls in enumerate(GRAD_CLASSES):
        for f in (2, 3, 4):
            for linear in (False, True):
                n = 1 + (i + f + int(linear)) % 2
                out.append((cls, f, n, 10 * f, 11 * f, channels_of(cls, f), linear, "synthetic"))
    out += [("dark_u8", 2, 1, 2, 2, 4, True, "synthetic"),     # one LR pixel
            ("wide_f32", 3, 2, 3, 3, 3, True, "synthetic"),
            ("white", 4, 1, 4, 4, 3, True, "synthetic")]
    for cls in ("noise_u8", "wide_f32"):
        for linear in (False, True):
            out.append((cls, 3, 2, 30, 33, channels_of(cls, 3, 1), linear, "imagenet"))
    return out


GRAD_CASES = _grad_cases()


def grad_case_id(case):
    cls, f, n, h, w, ch, linear, key = case
    return f"{cls}-f{f}-n{n}-{h}x{w}x{ch}-{'linear' if linear else 'plain'}-{key}"


def grad_case_batch(case):
    cls, f, n, h, w, ch, linear, key = case
    return make(cls, image_seed(cls, f, h, w) + 50 * n, n, h, w, ch)


# ---- end-to-end PSNR cases: (class, factor, h, w, channels, linear_loss, weights) ---------------------------------------------------------
# Not the constants: their error is the trained residual alone, ill-conditioned as above.  test_pixel_classes_cpu.py admits a row only
# where the oracle's own f32 and f64 PSNR agree within 0.001 dB.
PSNR_CLASSES = ("dark_u8", "bright_u8", "noise_u8", "wide_f32")
PSNR_CASES = [(cls, f, 12 * f + 1, 15 * f + 2, channels_of(cls, f), linear, key)
              for cls in PSNR_CLASSES for f, key in ((2, "synthetic"), (3, "synthetic"), (4, "synthetic"), (3, "imagenet"))
              for linear in (False, True)]


def psnr_case_id(case):
    cls, f, h, w, ch, linear, key = case
    return f"{cls}-f{f}-{h}x{w}x{ch}-{'linear' if linear else 'plain'}-{key}"


def psnr_case_image(case):
    cls, f, h, w, ch, linear, key = case
    return make(cls, image_seed(cls, f, h, w) + 3, 1, h, w, ch)[0]
