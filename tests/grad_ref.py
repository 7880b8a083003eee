"""A torch-f64 autograd restatement of the reference's training graph sr_net(f, Some((l2, linear_loss))) (src/network.rs:16-103),
written from network.rs and the op semantics of oracle/sr_oracle.c, not from rusty_sr_amd's kernels -- the yardstick of
include/srhip.h sr_backprop_* (tests/test_grad_restatement.py checks it against the C oracle and against finite differences;
tests/test_gpu_backprop.py holds the GPU to it).

  input  = LinearToSrgb(mean_fxf(SrgbToLinear(hr)))                  (the validation pass's pool; the top-left f*(h//f) x f*(w//f) crop)
  output = LinearInterp_f(input) + Expand_f(conv stack(input))       (network.rs:27-72)
  e      = output - hr, or SrgbToLinear(output) - SrgbToLinear(hr)   (linear_loss)
  loss   = loss_scale * sum e^2 + l2 * sum p^2                       (MseLoss / L2Regularisation conventions: UNPINNED, srhip.h)"""
import numpy as np
import torch
import torch.nn.functional as F

THRESH = float(np.float32(0.04045))   # the f32 constant the devices compare against


def segments(f):
    """name -> (offset, length, shape) of sr_net(f)'s parameters in .rsr order (oracle.SEGMENTS at f = 3)."""
    e = 3 * f * f
    spec = [("conv0", (32, 5, 5, 3)), ("f_bias", (32,)), ("f_activ", (32,)), ("expand_bias", (e,)), ("l1_bias", (32,)),
            ("l2_bias", (32,)), ("l3_bias", (32,)), ("l1_activ", (32,)), ("l2_activ", (32,)), ("l3_activ", (32,)),
            ("conv1", (32, 5, 5, 32)), ("conv2", (32, 5, 5, 32)), ("conv3", (32, 5, 5, 32)), ("conv5", (32, 3, 3, 32)),
            ("conv6", (32, 3, 3, 32)), ("conv7", (e, 3, 3, 32)), ("conv8", (32, 3, 3, 32)), ("conv9", (e, 3, 3, 32)),
            ("conv10", (e, 3, 3, 32))]
    out, off = {}, 0
    for name, shape in spec:
        n = int(np.prod(shape))
        out[name] = (off, n, shape)
        off += n
    return out


def num_params(f):
    s = segments(f)
    return s["conv10"][0] + s["conv10"][1]


def s2l(x):
    """SrgbToLinear, any real input (the linear segment below the threshold; clamped in the unused branch so autograd stays finite)."""
    return torch.where(x <= THRESH, x / 12.92, ((torch.clamp(x, min=0.04) + 0.055) / 1.055) ** 2.4)


def l2s(v):
    return torch.where(v <= 0.0031308, 12.92 * v, 1.055 * torch.clamp(v, min=0.0031) ** (1 / 2.4) - 0.055)


def hr_values(hr):
    """img_to_data (byte / 255 in f32, alpha dropped) or the f32 image as is; (..., 3) f64."""
    hr = np.asarray(hr)
    v = hr[..., :3].astype(np.float32) / np.float32(255) if hr.dtype == np.uint8 else hr.astype(np.float32)
    return torch.from_numpy(v.astype(np.float64))


def crop(hr64, f):
    h, w = hr64.shape[-3], hr64.shape[-2]
    return hr64[..., :f * (h // f), :f * (w // f), :]


def pool(hr64, f):
    """(n, h, w, 3) f64 -> (n, h//f, w//f, 3): LinearToSrgb of the f x f mean of SrgbToLinear."""
    c = crop(hr64, f)
    n, h, w, _ = c.shape
    lin = s2l(c).reshape(n, h // f, f, w // f, f, 3)
    return l2s(lin.mean(dim=(2, 4)))


def _interp_index(size, f):
    o = np.arange(size * f)
    y, py = o // f, o % f
    ny = 2 * py + 1 - f
    a = np.clip(y + np.where(ny < 0, -1, 0), 0, size - 1)
    b = np.clip(y + np.where(ny < 0, 0, 1), 0, size - 1)
    t = np.where(ny < 0, ny + 2 * f, ny) / (2.0 * f)
    return torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(t)


def linear_interp(x, f):
    """alumina LinearInterp x f (network.rs:27): half-pixel centres, clamped edges, on (n, H, W, 3)."""
    _, H, W, _ = x.shape
    ya, yb, ty = _interp_index(H, f)
    xa, xb, tx = _interp_index(W, f)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    ra, rb = x[:, ya], x[:, yb]
    va = (1 - tx) * ra[:, :, xa] + tx * ra[:, :, xb]
    vb = (1 - tx) * rb[:, :, xa] + tx * rb[:, :, xb]
    return (1 - ty) * va + ty * vb


def _belu(z, beta):
    return beta * z + torch.sqrt(z * z + 1.0) - 1.0


def forward(p, x, f):
    """sr_net(f)(x): p a flat f64 tensor (.rsr order), x (n, H, W, 3) f64 -> (n, fH, fW, 3)."""
    S = segments(f)
    g = {k: p[o:o + n].reshape(shape) for k, (o, n, shape) in S.items()}

    def conv(t, k):
        w = g[k].permute(0, 3, 1, 2)
        return F.conv2d(t, w, padding=w.shape[-1] // 2)

    def bias(k):
        return g[k].reshape(1, -1, 1, 1)

    xc = x.permute(0, 3, 1, 2)
    a0 = _belu(conv(xc, "conv0") + bias("f_bias"), bias("f_activ"))
    a1 = _belu(conv(a0, "conv1") + bias("l1_bias"), bias("l1_activ"))
    a2 = _belu(conv(a0, "conv2") + bias("l2_bias") + conv(a1, "conv5"), bias("l2_activ"))
    a3 = _belu(conv(a0, "conv3") + bias("l3_bias") + conv(a1, "conv6") + conv(a2, "conv8"), bias("l3_activ"))
    e = conv(a1, "conv7") + conv(a2, "conv9") + conv(a3, "conv10") + bias("expand_bias")
    n, _, H, W = e.shape
    # Expand (network.rs:39): channel (dy*f+dx)*3+c -> out[f y+dy][f x+dx][c]
    d2s = e.reshape(n, f, f, 3, H, W).permute(0, 4, 1, 5, 2, 3).reshape(n, f * H, f * W, 3)
    return linear_interp(x, f) + d2s


def loss(p, x, hr64, f, linear_loss=False, loss_scale=1.0, l2=0.0):
    """(scaled loss, err_sum) for LR input x (n, H, W, 3) and the HR crop hr64 (n, fH, fW, 3), both f64."""
    out = forward(p, x, f)
    e = (s2l(out) - s2l(hr64)) if linear_loss else (out - hr64)
    err = (e * e).sum()
    return loss_scale * err + l2 * (p * p).sum(), err


def backprop(params, hr, f, linear_loss=False, loss_scale=None, l2=0.0, x=None):
    """The gradient the GPU computes, in f64: hr (n, h, w, 3|4) u8 or (n, h, w, 3) f32; x: the pooled input to use (default: this
    module's f64 pool).  -> (err_sum, n_elems, grad f64 numpy)."""
    hr64 = hr_values(hr)
    if hr64.dim() == 3:
        hr64 = hr64[None]
    if x is None:
        x = pool(hr64, f)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    if x.dim() == 3:
        x = x[None]
    target = crop(hr64, f)
    if loss_scale is None:
        loss_scale = 1.0 / target.numel()
    p = torch.tensor(np.asarray(params, dtype=np.float64), requires_grad=True)
    total, err = loss(p, x, target, f, linear_loss, loss_scale, l2)
    total.backward()
    return float(err.detach()), target.numel(), p.grad.numpy()
