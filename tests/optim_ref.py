"""The optimiser's rules (include/srhip.h "Optimiser") restated in numpy: the gradient norm's order of additions, the clipping scale,
the parameter average and the learning-rate schedules.  The GPU tests hold the kernels to these bit for bit; test_optim_cpu.py holds
the restated sum to math.fsum within the bound its additions allow."""
import math

import numpy as np

_LANE = np.arange(64)


def wave_sum(v):
    """The butterfly of sr_reduce.h's wave_sum over the last axis (64 lanes): v + v[i ^ off] for off = 32 .. 1; every lane ends alike."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ off]
    return v


def block_sum(v):
    """block_sum of sr_reduce.h over the last axis (256 lanes): each wave's sum, then ((w0 + w1) + w2) + w3."""
    w = wave_sum(v.reshape(v.shape[:-1] + (4, 64)))[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def sumsq(g) -> np.float64:
    """S of sr_grad_norm_dev: partial b = block_sum of the squares of elements 256 b .. 256 b + 255 (0.0 past n); lane t of one workgroup
    adds partials t, t + 256, ... in order, and block_sum of the 256 lanes is S."""
    g = np.asarray(g, dtype=np.float32).ravel()
    n = g.size
    parts = (n + 255) // 256
    with np.errstate(all="ignore"):
        d = np.zeros(parts * 256, dtype=np.float64)
        d[:n] = g.astype(np.float64)
        part = block_sum((d * d).reshape(parts, 256))
        rounds = (parts + 255) // 256
        padded = np.zeros(rounds * 256, dtype=np.float64)   # (x + 0.0 is x for the sums of squares here: none is -0.0)
        padded[:parts] = part
        acc = np.zeros(256, dtype=np.float64)
        for r in range(rounds):
            acc = acc + padded[256 * r:256 * r + 256]
        return np.float64(block_sum(acc))


def norm_rule(S, clip):
    """(scale as f32, skip) from S and the f32 clip (0: no clipping)."""
    S, clip = np.float64(S), np.float32(clip)
    with np.errstate(all="ignore"):
        norm = np.sqrt(S)
        scale = np.float32(np.float64(clip) / norm) if clip > 0 and norm > np.float64(clip) else np.float32(1.0)
    return scale, int(not np.isfinite(S))


def grad_norm(g, clip):
    S = sumsq(g)
    scale, skip = norm_rule(S, clip)
    return {"sumsq": float(S), "scale": float(scale), "skip": skip}


def ema(e, p, decay):
    """e <- d e + (1.0f - d) p in f32, each product and the sum rounded on its own."""
    d = np.float32(decay)
    omd = np.float32(1.0) - d
    return (d * np.asarray(e, np.float32) + omd * np.asarray(p, np.float32)).astype(np.float32)


def lr_at(kind, base, step, warmup=0, every=0, gamma=0.0, total=0, min_lr=0.0) -> np.float32:
    """sr_lr_at in f64, rounded once to f32; base and min_lr are the f32 values the schedule struct holds."""
    base, mn, t = np.float64(np.float32(base)), np.float64(np.float32(min_lr)), np.float64(step)
    if kind == "constant":
        val = base
    elif kind == "step":
        val = base * np.power(np.float64(gamma), np.float64((step - 1) // every))
    elif kind == "cosine":
        T = np.float64(total)
        val = mn + (base - mn) * (np.float64(0.5) * (np.float64(1.0) + np.cos(np.float64(math.pi) * min(t - 1.0, T) / T)))
    else:
        raise ValueError(kind)
    warm = min(np.float64(1.0), t / np.float64(warmup)) if warmup else np.float64(1.0)
    return np.float32(warm * val)


NORM_SIZES = (1, 63, 64, 255, 256, 257, 1023, 65536, 65792)   # 65792 = 257 x 256: one partial more than the summing workgroup has lanes


def norm_vectors(n, seed=0):
    """The named test vectors of n floats (without the non-finite ones)."""
    rng = np.random.default_rng([seed, n])
    gauss = rng.standard_normal(n).astype(np.float32)
    wide = (gauss * np.float32(10.0) ** rng.integers(-30, 31, n).astype(np.float32)).astype(np.float32)  # magnitudes to 1e30
    return {"gauss": gauss, "zero": np.zeros(n, np.float32), "wide": wide}
