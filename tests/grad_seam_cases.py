"""The backward pass at its reduction seams (rusty_sr_amd/csrc/sr_grad.hip): the case table of tests/test_grad_seams_cpu.py and
tests/test_gpu_grad_seams.py, a Python restatement of the four rules by which layout() splits the NP = n H W LR pixels, and the builders
of the probe.  HIP-free.

The probe is an impulse of error.  x is a seeded random LR batch, hr the f64 restatement's own output for it rounded once to f32
(grad_ref.forward), and at each chosen LR pixel P the f x f x 3 HR samples that P owns get +-A (seeded signs).  Under the squared loss
with linear_loss = 0 the seed d_e = 2 s (out - hr) is then zero up to rounding everywhere but at P, the d_z maps are non-zero only in the
dependency cone around P (radius 5 for d_z of f; a weight gradient reads two pixels further), and every weight, bias and activation
gradient is made by the handful of pixels around P: one dropped, doubled or misread pixel beside a seam moves a segment by tens of per
cent of its norm, where on a smooth random image it moves it by less than the bar.  The rows run SR_LOSS_MSE only: the seed of L1 and
Charbonnier is a sign or a bounded ratio of the error, so the rounding noise of every other pixel would weigh as much as the impulse."""
import contextlib
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

import grad_ref
from param_families import bundled_scale as synthetic_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AMPLITUDE = 64.0   # A: f32 HR values are not confined to [0, 1], and under the squared loss everything is linear in A.  Two gates hold it to
                   # the rounding it has to stand out from: the f32 rounding of hr (tests/test_grad_seams_cpu.py: at A = 16 the impulse-
                   # free gradient reached 0.54e-3 .. 1.01e-3 of the bar, case A's corner pixel on the bundled weights just over the
                   # 1e-3 allowed, so A went up by 4) and the GPU's forward rounding (the noise gate of tests/test_gpu_grad_seams.py)
CONE = 15          # impulses of one call lie at least this far apart (Chebyshev, in LR pixels) unless they share a seam: disjoint cones
LOSS_SCALE = 1.0

# name -> factor, n, LR H, LR W and what layout() must give for it: (wchunks, wchunk), (cchunks, cchunk), conv_grid, loss_grid
CASES = {
    "A": dict(f=3, n=1, H=19, W=31, NP=589, w=(2, 295), c=(1, 589), conv=5, loss=3),         # odd chunk, seam in mid-row (row 9, column 16)
    "B": dict(f=2, n=3, H=13, W=19, NP=741, w=(2, 371), c=(1, 741), conv=6, loss=3),         # image seams inside a wave and inside a chunk
    "C": dict(f=4, n=1, H=29, W=37, NP=1073, w=(3, 358), c=(2, 537), conv=9, loss=5),        # two column-sum chunks (odd, 1 mod 4); E = 48
    "D": dict(f=2, n=1, H=211, W=311, NP=65621, w=(128, 513), c=(65, 1010), conv=513, loss=257),  # the cap on wchunks; last chunk 470 px
}


def split(n, H, W):
    """layout()'s four split rules, restated: the fields of the plan record's `grad` line."""
    NP = n * H * W
    wchunks = min(128, max(1, -(-NP // 512)))
    cchunks = min(256, max(1, -(-NP // 1024)))
    return dict(n=n, h=H, w=W, conv=-(-NP // 128), loss=-(-NP // 256), wchunks=wchunks, wchunk=-(-NP // wchunks), cchunks=cchunks,
                cchunk=-(-NP // cchunks))


def stands_on(p, g):
    """Where LR pixel p (flattened over the batch) sits relative to the seams of the split g (a `grad` line, or split()): a set of tags
    "<kernel>:<seam>:<side>".  The sides: `last` / `first` of the part before / after the seam; `unpaired` = the single pixel of a
    half-filled MFMA pair (an odd chunk's last pixel); `tail` = the pass's last pixel; `row3` .. = the column sum's row thread."""
    n, H, W = g["n"], g["h"], g["w"]
    HW, NP = H * W, n * H * W
    assert 0 <= p < NP
    tags = set()

    def seam(kernel, name, size):
        r = p % size
        if r == size - 1 and p + 1 < NP:
            tags.add(f"{kernel}:{name}:last")
        if r == 0 and p > 0:
            tags.add(f"{kernel}:{name}:first")

    seam("wgrad", "chunk", g["wchunk"])
    k = p // g["wchunk"]
    p0, p1 = k * g["wchunk"], min(NP, (k + 1) * g["wchunk"])
    if p == p1 - 1 and (p1 - p0) % 2 == 1:
        tags.add("wgrad:chunk:unpaired")
    if (p == p0 and p0 > 0 and p0 % W) or (p == p1 - 1 and p1 < NP and p1 % W):
        tags.add("wgrad:chunk:midrow")   # the seam beside p cuts a row in two
    if g["wchunks"] == 128 and g["wchunk"] > 512:
        tags.add("wgrad:capped")
    seam("colsum", "chunk", g["cchunk"])
    if any(t.startswith("colsum:chunk") for t in tags):
        tags.add(f"colsum:row{(p - p // g['cchunk'] * g['cchunk']) % 4}")
    seam("conv", "workgroup", 128)
    seam("conv", "wave", 32)
    seam("loss", "partial", 256)
    img, r = divmod(p, HW)
    if r == HW - 1 and img + 1 < n:
        tags.add("image:seam:last")
    if r == 0 and img > 0:
        tags.add("image:seam:first")
    if r >= HW - W and img + 1 < n:
        tags.add("image:lastrow")     # a tap below reads zero padding, not row 0 of the next image
    if r < W and img > 0:
        tags.add("image:firstrow")    # a tap above reads zero padding, not the last row of the image before
    if p == NP - 1:
        tags.add("tail")
    return tags


def _w(k, wchunk):
    return [(k * wchunk - 1, {"wgrad:chunk:last"}), (k * wchunk, {"wgrad:chunk:first"})]


# One row = one GPU call: (case, weights, linear_loss, ((pixel, the tags it must carry), ...)).  Cases A - C: a call per pixel.
def _rows():
    rows = []
    a = _w(1, 295) + [(127, {"conv:workgroup:last"}), (128, {"conv:workgroup:first"}), (255, {"loss:partial:last"}),
                      (256, {"loss:partial:first"}), (588, {"tail"})]
    a[0] = (294, {"wgrad:chunk:last", "wgrad:chunk:unpaired", "wgrad:chunk:midrow"})
    a[1] = (295, {"wgrad:chunk:first", "wgrad:chunk:midrow"})
    for weights in ("synthetic", "imagenet"):
        rows += [("A", weights, False, (px,)) for px in a]
    rows.append(("A", "synthetic", True, (a[0],)))
    b = [(370, {"wgrad:chunk:last", "wgrad:chunk:unpaired"}), (371, {"wgrad:chunk:first"}),
         (246, {"image:seam:last", "image:lastrow"}), (247, {"image:seam:first", "image:firstrow"}),
         (493, {"image:seam:last", "image:lastrow"}), (494, {"image:seam:first", "image:firstrow"}),
         (31, {"conv:wave:last"}), (32, {"conv:wave:first"})]
    rows += [("B", "synthetic", False, (px,)) for px in b]
    c = _w(1, 358) + _w(2, 358) + [(536, {"colsum:chunk:last", "colsum:row0"}), (537, {"colsum:chunk:first", "colsum:row0"})]
    rows += [("C", "synthetic", False, (px,)) for px in c]
    d = []
    for k in (1, 64, 127):
        d += [(k * 513 - 1, {"wgrad:chunk:last", "wgrad:chunk:unpaired", "wgrad:capped"}), (k * 513, {"wgrad:chunk:first", "wgrad:capped"})]
    for k in (1, 64):
        d += [(k * 1010 - 1, {"colsum:chunk:last", "colsum:row1"}), (k * 1010, {"colsum:chunk:first", "colsum:row0"})]
    d.append((65620, {"tail", "wgrad:capped"}))
    rows.append(("D", "synthetic", False, tuple(d)))
    return rows


ROWS = _rows()


def row_id(row):
    case, weights, linear, px = row
    where = "all" if len(px) > 1 else str(px[0][0])
    return f"{case}-{where}" + ("" if weights == "synthetic" else f"-{weights}") + ("-linear" if linear else "")


def pixels(row):
    return tuple(p for p, _ in row[3])


@functools.lru_cache(maxsize=None)
def weights_of(case, weights="synthetic"):
    f = CASES[case]["f"]
    if weights == "synthetic":
        return synthetic_params(f, 100 + f)
    assert f == 3
    import oracle
    with open(os.path.join(ROOT, "rusty_sr_amd", "res", weights + ".rsr"), "rb") as fh:
        return oracle.rsr_decode(fh.read())


@functools.lru_cache(maxsize=None)
def lr_batch(case):
    """the seeded random LR batch of a case, (n, H, W, 3) f32 in [0, 1)"""
    c = CASES[case]
    x = np.random.default_rng(4000 + ord(case)).random((c["n"], c["H"], c["W"], 3), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def base_hr(case, weights="synthetic"):
    """float32(grad_ref.forward(p, x, f)): the restatement's own output, rounded once -- the HR batch without any impulse"""
    f = CASES[case]["f"]
    with torch.no_grad():
        out = grad_ref.forward(torch.from_numpy(weights_of(case, weights).astype(np.float64)),
                               torch.from_numpy(lr_batch(case).astype(np.float64)), f)
    hr = out.numpy().astype(np.float32)
    hr.setflags(write=False)
    return hr


def hr_batch(case, weights, px, amplitude=AMPLITUDE):
    """base_hr with +-amplitude (signs seeded by the pixel) on the f x f x 3 samples each LR pixel of px owns"""
    c = CASES[case]
    f, H, W = c["f"], c["H"], c["W"]
    hr = base_hr(case, weights).copy()
    for p in px:
        img, r = divmod(p, H * W)
        y, x = divmod(r, W)
        sign = np.random.default_rng(9000 + p).choice(np.float32([-1.0, 1.0]), (f, f, 3))
        hr[img, f * y:f * y + f, f * x:f * x + f, :] += np.float32(amplitude) * sign
    return hr


CONV_ORDER = ("conv0", "conv1", "conv2", "conv5", "conv3", "conv6", "conv8", "conv7", "conv9", "conv10")  # grad_ref.forward's calls, in order


class _Tap:
    """stands in for torch.nn.functional inside grad_ref.forward: the same conv2d, its input kept and its output's gradient retained"""

    def __init__(self):
        self.calls = []

    def conv2d(self, t, w, padding=0):
        y = F.conv2d(t, w, padding=padding)
        y.retain_grad()
        self.calls.append((t, y))
        return y


@contextlib.contextmanager
def _tapped():
    tap, keep = _Tap(), grad_ref.F
    grad_ref.F = tap
    try:
        yield tap
    finally:
        grad_ref.F = keep


def restate(case, weights, linear, px, amplitude=AMPLITUDE, nodes=False):
    """grad_ref's loss and gradient on (lr_batch, hr_batch) at LOSS_SCALE, l2 = 0 -> (err, grad f64); nodes: also {conv: (its input
    (n, C, H, W), the gradient of its output (n, O, H, W))} as f64 numpy -- the d_z maps, and d_e as conv10's."""
    f = CASES[case]["f"]
    hr = hr_batch(case, weights, px, amplitude)
    if not nodes:
        err, _, g = grad_ref.backprop(weights_of(case, weights), hr, f, linear, LOSS_SCALE, 0.0, x=lr_batch(case).astype(np.float64))
        return err, g
    p = torch.tensor(weights_of(case, weights).astype(np.float64), requires_grad=True)
    with _tapped() as tap:
        total, err = grad_ref.loss(p, torch.from_numpy(lr_batch(case).astype(np.float64)), grad_ref.hr_values(hr), f, linear, LOSS_SCALE, 0.0)
    total.backward()
    assert len(tap.calls) == len(CONV_ORDER)
    kept = {name: (t.detach().numpy(), y.grad.numpy()) for name, (t, y) in zip(CONV_ORDER, tap.calls)}
    return float(err.detach()), p.grad.numpy(), kept


@functools.lru_cache(maxsize=None)
def reference(case, weights, linear, px, amplitude=AMPLITUDE):
    """restate(), computed once per row and shared"""
    err, g = restate(case, weights, linear, px, amplitude)
    g.setflags(write=False)
    return err, g


def norm_bar(want_seg):
    """the norm bar of test_gpu_backprop.assert_grad_close for one segment of the wanted gradient (tests/test_grad_seams_cpu.py holds this
    restatement to the assertion itself)"""
    want_seg = np.asarray(want_seg, dtype=np.float64)
    return 1e-4 * np.linalg.norm(want_seg) + 1e-7 * np.abs(want_seg).max()


def pixel_term(kept, name, p, H, W, wrap=False):
    """One pixel's term of a convolution's weight gradient, dy[p] (x) x[p + tap], as [O][KH][KW][I] f64.  wrap: instead, what the taps
    outside p's own image would add if they read on in the flattened batch (the neighbouring image's rows) and not zero padding."""
    xin, dy = kept[name]
    n, C = xin.shape[0], xin.shape[1]
    O = dy.shape[1]
    ks = 5 if name in ("conv0", "conv1", "conv2", "conv3") else 3
    pad = ks // 2
    img, r = divmod(p, H * W)
    y, x = divmod(r, W)
    flat = xin.transpose(0, 2, 3, 1).reshape(n * H, W, C)   # rows of the whole batch, image after image
    out = np.zeros((O, ks, ks, C))
    for kh in range(ks):
        yy = y + kh - pad
        inside = 0 <= yy < H
        row = img * H + yy
        if inside == wrap or not 0 <= row < n * H:
            continue
        for kw in range(ks):
            xx = x + kw - pad
            if 0 <= xx < W:
                out[:, kh, kw, :] = np.outer(dy[img, :, y, x], flat[row, xx])
    return out
