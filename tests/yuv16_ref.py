"""The colour rule of the deep video path (include/srhip.h "Deep video") restated in numpy, f64: planar YCbCr frames of 9..16-bit samples
held in little-endian uint16, laid out like a Y4M frame payload, to the network's f32 RGB input and back from its unquantised f32 output.
It is tests/yuv_ref.py generalised to a depth d, with 4:2:2 and BT.2020 (non-constant luminance) added.  This file is the definition;
the kernels of rusty_sr_amd/csrc/sr_yuv.hip on uint16 samples are held to it sample for sample and bit for bit (tests/test_gpu_video_deep.py), and
tests/test_yuv16_cpu.py holds the rule itself to its properties and to the 8-bit rule.

Every expression below is one IEEE operation per numpy call, in the order the header writes it.  A code is the uint16 as stored,
whatever d says: nothing is masked, and the clamp of RGB to [0, 1] defines every input."""
import numpy as np

import yuv_ref

SUBSAMPLINGS = ("420", "422", "444")
SITINGS = ("center", "left")
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
RANGES = ("limited", "full")
DEPTHS = tuple(range(9, 17))
FORMS = (("420", "center"), ("420", "left"), ("422", "center"), ("422", "left"), ("444", "center"))


class Rule:
    """The constants of a format at depth d, each formed once by a single operation (the host side of the library forms the same)."""

    def __init__(self, matrix="bt709", range="limited", depth=10):
        assert depth in DEPTHS
        kr, kb = (np.float64(v) for v in MATRICES[matrix])
        one, two = np.float64(1.0), np.float64(2.0)
        self.kr, self.kb = kr, kb
        self.kg = one - kr - kb
        self.cr2, self.cb2 = two * (one - kr), two * (one - kb)
        self.ib, self.ir, self.ig = one / self.cb2, one / self.cr2, one / self.kg
        s = np.float64(2.0 ** (depth - 8))
        top = np.float64(2.0 ** depth) - one
        if range == "full":
            self.oy, self.ky, self.kc, self.mid = np.float64(0.0), top, top, np.float64(2.0 ** (depth - 1))
            self.ylim = self.clim = (0.0, float(top))
        else:
            self.oy, self.ky, self.kc, self.mid = np.float64(16.0) * s, np.float64(219.0) * s, np.float64(224.0) * s, np.float64(128.0) * s
            self.ylim = (float(np.float64(16.0) * s), float(np.float64(235.0) * s))
            self.clim = (float(np.float64(16.0) * s), float(np.float64(240.0) * s))
        self.sy, self.sc = one / self.ky, one / self.kc
        self.depth = depth


def plane_shapes(sub, h, w):
    """((h, w), (ch, cw)): the luma plane and either chroma plane."""
    if sub == "420":
        return (h, w), ((h + 1) // 2, (w + 1) // 2)
    if sub == "422":
        return (h, w), (h, (w + 1) // 2)
    return (h, w), (h, w)


def frame_samples(sub, h, w):
    (_, _), (ch, cw) = plane_shapes(sub, h, w)
    return h * w + 2 * ch * cw


def frame_bytes(sub, h, w):
    return 2 * frame_samples(sub, h, w)


def split(frame, sub, h, w):
    """A frame's samples (frame_samples of them, uint16) -> its Y, Cb, Cr planes (views)."""
    frame = np.asarray(frame, dtype=np.uint16).reshape(-1)
    (_, _), (ch, cw) = plane_shapes(sub, h, w)
    assert frame.size == frame_samples(sub, h, w)
    y = frame[:h * w].reshape(h, w)
    cb = frame[h * w:h * w + ch * cw].reshape(ch, cw)
    cr = frame[h * w + ch * cw:].reshape(ch, cw)
    return y, cb, cr


def join(y, cb, cr):
    return np.concatenate([np.asarray(p, dtype=np.uint16).reshape(-1) for p in (y, cb, cr)])


def upsample_chroma_422(c, w, siting):
    """A 4:2:2 chroma plane at luma resolution, as the exact integers 4 x value: the horizontal taps of yuv_ref alone."""
    c = np.asarray(c, dtype=np.int64)
    xa, xb, wxa, wxb = yuv_ref._taps_2x(w, c.shape[1], siting == "center")
    return c[:, xa] * wxa[None, :] + c[:, xb] * wxb[None, :]


def yuv_to_rgb(frame, h, w, sub="420", siting="left", matrix="bt709", range="limited", depth=10):
    """One frame's samples -> (h, w, 3) f32 RGB in [0, 1]."""
    k = Rule(matrix, range, depth)
    yp, cbp, crp = split(frame, sub, h, w)
    if sub == "420":
        cb = yuv_ref.upsample_chroma(cbp, h, w, siting).astype(np.float64) * np.float64(0.0625)
        cr = yuv_ref.upsample_chroma(crp, h, w, siting).astype(np.float64) * np.float64(0.0625)
    elif sub == "422":
        cb = upsample_chroma_422(cbp, w, siting).astype(np.float64) * np.float64(0.25)
        cr = upsample_chroma_422(crp, w, siting).astype(np.float64) * np.float64(0.25)
    else:
        cb, cr = cbp.astype(np.float64), crp.astype(np.float64)
    y = (yp.astype(np.float64) - k.oy) * k.sy
    cb = (cb - k.mid) * k.sc
    cr = (cr - k.mid) * k.sc
    r = y + k.cr2 * cr
    b = y + k.cb2 * cb
    g = ((y - k.kr * r) - k.kb * b) * k.ig
    rgb = np.stack([r, g, b], axis=-1)
    return np.clip(rgb, 0.0, 1.0).astype(np.float32)


def _round_code(v, lim):
    return np.clip(np.floor(v + np.float64(0.5)), lim[0], lim[1]).astype(np.uint16)


def rgb_to_yuv(rgb, sub="420", siting="left", matrix="bt709", range="limited", depth=10):
    """(h, w, 3) f32 RGB of any magnitude (NaN counts as 0) -> the frame's samples (uint16)."""
    k = Rule(matrix, range, depth)
    with np.errstate(invalid="ignore"):
        x = np.asarray(rgb, dtype=np.float32).astype(np.float64)
        h, w, _ = x.shape
        x = np.where(x > 0.0, x, 0.0)        # NaN and everything below 0 -> 0
        x = np.where(x < 1.0, x, 1.0)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    y = (k.kr * r + k.kg * g) + k.kb * b
    cb = (b - y) * k.ib
    cr = (r - y) * k.ir
    yq = k.oy + k.ky * y
    planes = [k.mid + k.kc * cb, k.mid + k.kc * cr]
    if sub != "444":
        (_, _), (ch, cw) = plane_shapes(sub, h, w)
        j = np.arange(cw)
        cm, c0, c1 = np.clip(2 * j - 1, 0, w - 1), np.clip(2 * j, 0, w - 1), np.clip(2 * j + 1, 0, w - 1)
        r0, r1 = np.clip(2 * np.arange(ch), 0, h - 1), np.clip(2 * np.arange(ch) + 1, 0, h - 1)
        out = []
        for p in planes:
            left = lambda rows: ((rows[:, cm] + np.float64(2.0) * rows[:, c0]) + rows[:, c1]) * np.float64(0.25)
            if sub == "422":
                v = (p[:, c0] + p[:, c1]) * np.float64(0.5) if siting == "center" else left(p)
            elif siting == "center":
                v = ((p[r0][:, c0] + p[r0][:, c1]) + (p[r1][:, c0] + p[r1][:, c1])) * np.float64(0.25)
            else:
                v = (left(p[r0]) + left(p[r1])) * np.float64(0.5)
            out.append(v)
        planes = out
    return join(_round_code(yq, k.ylim), _round_code(planes[0], k.clim), _round_code(planes[1], k.clim))
