"""The metrics of include/srhip.h ("Metrics"), restated in numpy: the integer BT.601 luma, the shave, the separable f64 SSIM with its
"valid" window positions, and the per-image aggregate.  The GPU tests compare the library with this; the CPU tests check this against an
independent 2-D evaluation."""
import math

import numpy as np

C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2


def weights():
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    return g / g.sum()


def luma(img):
    """(.., 3|4) u8 -> the 8-bit luma, int64: (65481 R + 128553 G + 24966 B + 127500) div 255000 + 16."""
    p = np.asarray(img)[..., :3].astype(np.int64)
    return (65481 * p[..., 0] + 128553 * p[..., 1] + 24966 * p[..., 2] + 127500) // 255000 + 16


def shaved(y, s):
    """The region left by removing s pixels from every border (empty where nothing is left)."""
    h, w = y.shape
    if s < 0:
        raise ValueError("shave must not be negative")
    if h - 2 * s <= 0 or w - 2 * s <= 0:
        return y[:0, :0]
    return y[s:h - s, s:w - s]


def filt(x, g):
    """Rows, then columns, 'valid' positions only: (H, W) f64 -> (H - 10, W - 10)."""
    rows = sum(g[k] * x[:, k:x.shape[1] - 10 + k] for k in range(11))
    return sum(g[k] * rows[k:x.shape[0] - 10 + k] for k in range(11))


def ssim_map(ya, yb):
    """The SSIM map of two luma regions with both sides >= 11, f64."""
    a, b, g = ya.astype(np.float64), yb.astype(np.float64), weights()
    ma, mb = filt(a, g), filt(b, g)
    va, vb, cov = filt(a * a, g) - ma * ma, filt(b * b, g) - mb * mb, filt(a * b, g) - ma * mb
    return ((2.0 * (ma * mb) + C1) * (2.0 * cov + C2)) / ((ma * ma + mb * mb + C1) * (va + vb + C2))


def metrics(a, b, shave):
    """Two (H, W, 3|4) u8 images -> the dict Engine.image_metrics returns."""
    ya, yb = shaved(luma(a), shave), shaved(luma(b), shave)
    d = ya - yb
    out = {"y_sq_err": int((d * d).sum()), "y_count": int(ya.size), "ssim_sum": 0.0, "ssim_count": 0}
    if ya.shape[0] >= 11 and ya.shape[1] >= 11:
        m = ssim_map(ya, yb)
        out["ssim_sum"], out["ssim_count"] = float(m.sum()), int(m.size)
    out["y_psnr"] = y_psnr(out["y_sq_err"], out["y_count"])
    out["ssim"] = None if out["ssim_count"] == 0 else out["ssim_sum"] / out["ssim_count"]
    return out


def y_psnr(y_sq_err, y_count):
    if y_count == 0:
        return None
    return math.inf if y_sq_err == 0 else 10.0 * math.log10(255.0 ** 2 * y_count / y_sq_err)


def aggregate(per_image):
    """Per-image dicts with err_sum, n_elems, y_psnr, ssim -> the pooled PSNR, the means of the per-image scores (inf where an image has
    no error), and the (index, score) pairs the means leave out."""
    err, n = sum(m["err_sum"] for m in per_image), sum(m["n_elems"] for m in per_image)
    ys = [m["y_psnr"] for m in per_image if m["y_psnr"] is not None]
    ss = [m["ssim"] for m in per_image if m["ssim"] is not None]
    skipped = [(i, k) for i, m in enumerate(per_image) for k in ("y_psnr", "ssim") if m[k] is None]
    return {"psnr": math.inf if err == 0 else -10.0 * math.log10(err / n), "y_psnr": sum(ys) / len(ys) if ys else None,
            "ssim": sum(ss) / len(ss) if ss else None, "skipped": skipped}
