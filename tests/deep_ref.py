"""The deep-colour rule (include/srhip.h "Deep colour") restated in numpy: 16-bit samples to the network's f32 input and the network's
f32 output back to 16-bit samples.  UNPINNED: the reference has no counterpart (its images are 8 bits wide).  Every operation is one
f32 operation, in the written order -- numpy rounds each to f32, as the kernels do without contraction -- so the kernels are held to
this bit for bit (tests/test_gpu_deep.py); the properties of the rule itself are tests/test_deep_cpu.py's."""
import numpy as np

F = np.float32
LEVELS = 65536
TOP = F(65535.0)


def to_f32(px, in_channels=None):
    """uint16 samples (..., C), C in 1..4 -> (..., 3) f32: v / 65535, one IEEE f32 division; grey (1 or 2 channels) is copied to
    R = G = B, alpha (the last of 2 or 4 channels) is dropped."""
    px = np.asarray(px)
    assert px.dtype == np.uint16
    c = px.shape[-1] if in_channels is None else in_channels
    assert px.shape[-1] == c and 1 <= c <= 4
    x = px.astype(F) / TOP
    if c <= 2:
        return np.repeat(x[..., :1], 3, axis=-1)
    return np.ascontiguousarray(x[..., :3])


def quantise_values(v):
    """f32 values -> uint16: floor(65535 v + 0.5) clamped to 0 .. 65535, the product and the sum each rounded to f32; NaN -> 0."""
    v = np.asarray(v, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor(TOP * v + F(0.5))
        t = np.fmin(np.fmax(t, F(0.0)), TOP)   # fmax / fmin give the other argument for a NaN, as fmaxf / fminf do
    assert t.dtype == F
    return t.astype(np.uint16)


def grey(x):
    """(..., 3) f32 -> (...) f32: ((r + g) + b) / 3, each operation in f32."""
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((x[..., 0] + x[..., 1]) + x[..., 2]) / F(3.0)


def quantise(x, out_channels=3):
    """(..., 3) f32 -> (..., out_channels) uint16: 3 RGB16, 4 RGBA16 with alpha 65535, 1 the grey mean quantised."""
    x = np.asarray(x, dtype=F)
    assert x.shape[-1] == 3 and out_channels in (1, 3, 4)
    if out_channels == 1:
        return quantise_values(grey(x))[..., None]
    q = quantise_values(x)
    if out_channels == 4:
        q = np.concatenate([q, np.full(q.shape[:-1] + (1,), 65535, np.uint16)], axis=-1)
    return q
