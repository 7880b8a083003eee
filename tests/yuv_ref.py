"""The colour rule of the video path (include/srhip.h "Video") restated in numpy, f64: planar 8-bit YCbCr frames, laid out like a Y4M
frame payload, to the network's f32 RGB input and back from its unquantised f32 output.  This file is the definition; the kernels of
rusty_sr_amd/csrc/sr_yuv.hip are held to it byte for byte and bit for bit (tests/test_gpu_video.py), and tests/test_yuv_cpu.py holds
the rule itself to its properties and to Pillow.

Every expression below is one IEEE operation per numpy call, in the order the header writes it: numpy never contracts a multiply and
an add, and the library is built without contraction."""
import numpy as np

SUBSAMPLINGS = ("420", "444")
SITINGS = ("center", "left")
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")


class Rule:
    """The constants of a format, each formed once by a single operation per step (the host side of the library forms the same)."""

    def __init__(self, matrix="bt601", range="limited"):
        kr, kb = (np.float64(v) for v in MATRICES[matrix])
        one, two = np.float64(1.0), np.float64(2.0)
        self.kr, self.kb = kr, kb
        self.kg = one - kr - kb
        self.cr2, self.cb2 = two * (one - kr), two * (one - kb)
        self.ib, self.ir, self.ig = one / self.cb2, one / self.cr2, one / self.kg
        full = range == "full"
        self.sy = one / np.float64(255.0 if full else 219.0)
        self.sc = one / np.float64(255.0 if full else 224.0)
        self.oy = np.float64(0.0 if full else 16.0)
        self.ky = np.float64(255.0 if full else 219.0)
        self.kc = np.float64(255.0 if full else 224.0)
        self.ylim = (0.0, 255.0) if full else (16.0, 235.0)
        self.clim = (0.0, 255.0) if full else (16.0, 240.0)


def plane_shapes(sub, h, w):
    """((h, w), (ch, cw)): the luma plane and either chroma plane."""
    if sub == "420":
        return (h, w), ((h + 1) // 2, (w + 1) // 2)
    return (h, w), (h, w)


def frame_bytes(sub, h, w):
    (_, _), (ch, cw) = plane_shapes(sub, h, w)
    return h * w + 2 * ch * cw


def split(frame, sub, h, w):
    """A frame's bytes (frame_bytes of them) -> its Y, Cb, Cr planes (views)."""
    frame = np.asarray(frame, dtype=np.uint8).reshape(-1)
    (_, _), (ch, cw) = plane_shapes(sub, h, w)
    assert frame.size == frame_bytes(sub, h, w)
    y = frame[:h * w].reshape(h, w)
    cb = frame[h * w:h * w + ch * cw].reshape(ch, cw)
    cr = frame[h * w + ch * cw:].reshape(ch, cw)
    return y, cb, cr


def join(y, cb, cr):
    return np.concatenate([np.asarray(p, dtype=np.uint8).reshape(-1) for p in (y, cb, cr)])


def _taps_2x(n_out, n_in, centred):
    """Per output index of an axis upsampled by two: (index a, index b, weight a, weight b), indices clamped, weights summing to 4."""
    o = np.arange(n_out)
    i = o // 2
    even = (o % 2) == 0
    if centred:
        a = np.where(even, i - 1, i)
        b = np.where(even, i, i + 1)
        wa = np.where(even, 1, 3)
        wb = np.where(even, 3, 1)
    else:  # co-sited with the even samples
        a, b = i, np.where(even, i, i + 1)
        wa, wb = np.where(even, 4, 2), np.where(even, 0, 2)
    return np.clip(a, 0, n_in - 1), np.clip(b, 0, n_in - 1), wa, wb


def upsample_chroma(c, h, w, siting):
    """A 4:2:0 chroma plane at luma resolution, as the exact integers 16 x value (bilinear; vertically centred under either siting)."""
    c = np.asarray(c, dtype=np.int64)
    ya, yb, wya, wyb = _taps_2x(h, c.shape[0], True)
    xa, xb, wxa, wxb = _taps_2x(w, c.shape[1], siting == "center")
    rows = lambda r: c[r][:, xa] * wxa[None, :] + c[r][:, xb] * wxb[None, :]
    return rows(ya) * wya[:, None] + rows(yb) * wyb[:, None]


def yuv_to_rgb(frame, h, w, sub="420", siting="center", matrix="bt601", range="limited"):
    """One frame's bytes -> (h, w, 3) f32 RGB in [0, 1]."""
    k = Rule(matrix, range)
    yp, cbp, crp = split(frame, sub, h, w)
    if sub == "420":
        cb = upsample_chroma(cbp, h, w, siting).astype(np.float64) * np.float64(0.0625)
        cr = upsample_chroma(crp, h, w, siting).astype(np.float64) * np.float64(0.0625)
    else:
        cb, cr = cbp.astype(np.float64), crp.astype(np.float64)
    y = (yp.astype(np.float64) - k.oy) * k.sy
    cb = (cb - np.float64(128.0)) * k.sc
    cr = (cr - np.float64(128.0)) * k.sc
    r = y + k.cr2 * cr
    b = y + k.cb2 * cb
    g = ((y - k.kr * r) - k.kb * b) * k.ig
    rgb = np.stack([r, g, b], axis=-1)
    return np.clip(rgb, 0.0, 1.0).astype(np.float32)


def _round_byte(v, lim):
    return np.clip(np.floor(v + np.float64(0.5)), lim[0], lim[1]).astype(np.uint8)


def rgb_to_yuv(rgb, sub="420", siting="center", matrix="bt601", range="limited"):
    """(h, w, 3) f32 RGB of any finite magnitude (NaN counts as 0) -> the frame's bytes."""
    k = Rule(matrix, range)
    x = np.asarray(rgb, dtype=np.float32).astype(np.float64)
    h, w, _ = x.shape
    x = np.where(x > 0.0, x, 0.0)        # NaN and everything below 0 -> 0
    x = np.where(x < 1.0, x, 1.0)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (k.kr * r + k.kg * g) + k.kb * b
    cb = (b - y) * k.ib
    cr = (r - y) * k.ir
    yq = k.oy + k.ky * y
    planes = [np.float64(128.0) + k.kc * cb, np.float64(128.0) + k.kc * cr]
    if sub == "420":
        (_, _), (ch, cw) = plane_shapes(sub, h, w)
        r0, r1 = np.clip(2 * np.arange(ch), 0, h - 1), np.clip(2 * np.arange(ch) + 1, 0, h - 1)
        j = np.arange(cw)
        cm, c0, c1 = np.clip(2 * j - 1, 0, w - 1), np.clip(2 * j, 0, w - 1), np.clip(2 * j + 1, 0, w - 1)
        out = []
        for p in planes:
            if siting == "center":
                v = ((p[r0][:, c0] + p[r0][:, c1]) + (p[r1][:, c0] + p[r1][:, c1])) * np.float64(0.25)
            else:
                row = lambda rr: ((p[rr][:, cm] + np.float64(2.0) * p[rr][:, c0]) + p[rr][:, c1]) * np.float64(0.25)
                v = (row(r0) + row(r1)) * np.float64(0.5)
            out.append(v)
        planes = out
    return join(_round_byte(yq, k.ylim), _round_byte(planes[0], k.clim), _round_byte(planes[1], k.clim))


def upscaled_frame_shape(h, w, f):
    return f * h, f * w
