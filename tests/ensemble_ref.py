"""The self-ensemble of include/srhip.h (sr_upscale_ensemble_*), restated in numpy: the 8 flips and rotations, their inverses, and the
f32 accumulation in the order the header fixes.  The GPU tests compare the library with this; the CPU tests check this against itself."""
import numpy as np


def T(x, k):
    """Member k (0..7) of an (h, w, C) image: swap the spatial axes if k & 4, then reverse the rows if k & 2, then the columns if k & 1."""
    if k & 4:
        x = np.swapaxes(x, 0, 1)
    if k & 2:
        x = x[::-1]
    if k & 1:
        x = x[:, ::-1]
    return np.ascontiguousarray(x)


def T_inv(y, k):
    """Undo T(., k): the same steps in the opposite order."""
    if k & 1:
        y = y[:, ::-1]
    if k & 2:
        y = y[::-1]
    if k & 4:
        y = np.swapaxes(y, 0, 1)
    return np.ascontiguousarray(y)


def members_of(mask):
    return [k for k in range(8) if mask >> k & 1]


def accumulate(outputs, count):
    """outputs: T_inv(forward(T(x, k)), k) as f32 arrays, in ascending k.  acc = 0.0f; acc = acc + o (plain f32 adds, in order);
    acc * (1.0f / count), the reciprocal formed in f32."""
    acc = np.zeros_like(outputs[0], dtype=np.float32)
    for o in outputs:
        acc = acc + o.astype(np.float32)
    return acc * (np.float32(1) / np.float32(count))


def ensemble(forward, x, members):
    """forward: (h, w, 3) f32 -> (f h, f w, 3); the result is f32 whatever forward returns."""
    ks = members_of(members)
    if not ks or members > 255:
        raise ValueError("members must have 1..8 of the bits 0..7")
    return accumulate([T_inv(np.asarray(forward(T(x, k)), dtype=np.float32), k) for k in ks], len(ks))


def quantise(v):
    """data_to_img: clamp(floor(255 v + 0.5)) in f32, alpha 255 -> (.., 4) u8."""
    q = np.clip(np.floor(v.astype(np.float32) * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
