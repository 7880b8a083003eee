"""Host-side mirror of the reference's engine seam for the upscale path.

Reference call site (src/main.rs:161-171):
    assert_eq!(params.len(), graph.num_params(), ...);
    let mut input = NodeData::new_blank(DataShape::new(CHANNELS, &[W, H], 1));
    img_to_data(&mut input.values, &input_image);
    let output = graph.forward(1, vec![input], &params).remove(0);
Here `sr_net(factor)` returns a Graph whose forward() runs the hand-written
gfx950 kernels through libsrhip's C ABI.  torch is used only for device memory
and streams."""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib

FACTOR = 3    # reference main.rs:31
CHANNELS = 3  # reference network.rs:13


@dataclass
class DataShape:
    """alumina DataShape::new(channels, &[W, H], n) (reference main.rs:168)."""
    channels: int
    spatial_dimensions: Sequence[int]  # [W, H]
    n: int = 1

    def flat_size_single(self):
        w, h = self.spatial_dimensions
        return self.channels * w * h


@dataclass
class NodeData:
    """alumina NodeData { shape, values } -- values are n x [y][x][c] f32."""
    shape: DataShape
    values: np.ndarray = field(default=None)

    @staticmethod
    def new_blank(shape: DataShape) -> "NodeData":
        return NodeData(shape, np.zeros(shape.n * shape.flat_size_single(), dtype=np.float32))


def img_to_data(pixels: np.ndarray) -> np.ndarray:
    """alumina supplier::imagefolder::img_to_data (reference main.rs:170):
    u8 RGB(A) -> f32 = u8/255, alpha dropped.  Host-side convenience for the
    f32 entry points; the rgba8 entry points fuse this into the first kernel."""
    px = np.asarray(pixels)
    if px.dtype != np.uint8 or px.shape[-1] not in (3, 4):
        raise ValueError("expected u8 pixels with 3 or 4 channels")
    return px[..., :3].astype(np.float32) / np.float32(255.0)


def parse_plan(text: str) -> dict:
    """A plan record (the text of sr_get_experiment "plan") as data:
    {"host": [(kind, [sizes], (y_lo, y_hi) | None)], "fork": [(forked, rows_a, rows_b)], "launches": [dict, ...], "aux": [dict, ...],
    "ops": [dict, ...]}.
    host kind: "one" | "batch" (sizes: images per chunk) | "inorder" | "alternating" (sizes: band rows).  A launch:
    st, form ("first" | "pipe"), ty8, ty4, grid, prec, f, img, out, ch, count (identical launches in a row).  An aux launch (the
    parameter-free graphs): graph, img, ch, grid, units, count; it is multi-round exactly when units > grid.  An op (a launch of a pixel
    operator: pad, crop, bleed, merge, resize_h, resize_v, resize_v_yuv (its grid: 1024 columns x 2 or 4 rows a workgroup), yuv2rgb, rgb2yuv, u16_to_f32, f32_to_u16, yuv16_to_rgb, rgb_to_yuv16, rows_differ (bx: its workgroups), in the order
    they were queued): name,
    px ("u8" | "f32": the pixels the kernel is instantiated on -- resize_h its input's, resize_v its output's, the two video conversions
    their input's, the two deep-colour and the two deep video conversions their f32 side), n, bx, by (workgroups along a row and along the rows of one image;
    resize_h: groups of the batch's n h rows; the deep-colour conversions: n = by = 1, the batch is one run of pixels), count, and form
    ("staged4" | "staged1" | "direct", resize_h; "420center" | "420left" | "444", the video conversions, and also
    "422center" | "422left", the deep video conversions; "wide" | "wide_in" | "wide_out" |
    "narrow", the deep-colour conversions) or f (the factor, merge).
    A record that holds a backward pass has one more key, "grad": a dict per pass (sr_grad_queue) of how it split its sums over the
    NP = n h w LR pixels -- n, h, w, conv (workgroups of 128 pixels), loss (f64 partials of 256 pixels each), wchunks x wchunk (weight-
    gradient chunks and their pixels), cchunks x cchunk (expand-bias column-sum chunks), count.  Other records have no such key.
    Lines of any other kind are ignored."""
    rec = {"host": [], "fork": [], "launches": [], "aux": [], "ops": []}
    for line in text.splitlines():
        words = line.split()
        count = 1
        if words[-1].startswith("x") and words[-1][1:].isdigit():
            count = int(words.pop()[1:])
        if words[0] == "host":
            rows = None
            if words[-1].startswith("rows="):
                a, b = words.pop()[5:].split(":")
                rows = (int(a), int(b))
            for _ in range(count):
                rec["host"].append((words[1], [int(v) for v in words[2].split(",")], rows))
        elif words[0] == "fork":
            sizes = [int(v) for v in words[2].split(",")] if len(words) > 2 and words[2][0].isdigit() else [0, 0]
            for _ in range(count):
                rec["fork"].append((words[1] == "1", sizes[0], sizes[1]))
        elif words[0] == "launch":
            d = dict(w.split("=", 1) for w in words[1:])
            for k in ("st", "ty8", "ty4", "grid", "f", "ch"):
                d[k] = int(d[k])
            d["count"] = count
            rec["launches"].append(d)
        elif words[0] == "aux":
            d = dict(w.split("=", 1) for w in words[1:])
            for k in ("ch", "grid", "units"):
                d[k] = int(d[k])
            d["count"] = count
            rec["aux"].append(d)
        elif words[0] == "op":
            d = dict(w.split("=", 1) for w in words[1:])
            for k in ("n", "bx", "by", "f"):
                if k in d:
                    d[k] = int(d[k])
            d["count"] = count
            rec["ops"].append(d)
        elif words[0] == "grad":
            d = {k: int(v) for k, v in (w.split("=", 1) for w in words[1:])}
            d["count"] = count
            rec.setdefault("grad", []).append(d)
    return rec


class Engine:
    """One sr_ctx (= one GPU, one parameter set)."""

    PRECISIONS = {"f32": _lib.SR_PRECISION_F32, "split_f16": _lib.SR_PRECISION_SPLIT_F16}

    GRAPHS = {"sr_net": _lib.SR_GRAPH_SR_NET, "bilinear": _lib.SR_GRAPH_BILINEAR, "downsample": _lib.SR_GRAPH_DOWNSAMPLE}

    def __init__(self, params=(), device: int = 0, factor: int = FACTOR, precision: str = "f32", graph: str = "sr_net"):
        L = _lib.lib()
        p = np.ascontiguousarray(params, dtype=np.float32)
        self._ctx = C.c_void_p()
        self.graph = graph
        self.factor = factor
        _lib.check(L.sr_create_graph(C.byref(self._ctx), self.GRAPHS[graph],
                                     p.ctypes.data_as(C.POINTER(C.c_float)) if p.size else None, p.size, factor, device))
        self.device = device
        self._L = L
        self.set_precision(precision)

    def set_precision(self, precision: str):
        """"f32": exact-f32 MFMA (default).  "split_f16": hi/lo half pairs, 3 f16 MFMAs per product."""
        _lib.check(self._L.sr_set_precision(self._ctx, self.PRECISIONS[precision]))
        self.precision = precision

    LOSSES = {"mse": _lib.SR_LOSS_MSE, "l1": _lib.SR_LOSS_L1, "charbonnier": _lib.SR_LOSS_CHARBONNIER}

    def set_loss(self, kind: str = "mse", eps: float = 1e-3):
        """sr_set_loss: the objective of every backward pass queued on this engine from now on -- backprop*, backprop_pair* and every
        step of a Trainer on it.  "mse" (the reference's sum of squares, the default), "l1", or "charbonnier" with 0 < eps <= 1
        (sqrt(e^2 + eps^2) - eps; eps is read for that kind alone).  Steps already queued keep the objective they were queued under.
        err_sum stays the sum of squares; validation, metrics and inference do not look at it.  A bad name or eps is a ValueError
        before the library is called."""
        if kind not in self.LOSSES:
            raise ValueError(f"loss: expected one of {', '.join(sorted(self.LOSSES))}, got {kind!r}")
        e = _check_loss_eps(eps) if kind == "charbonnier" else 0.0
        _lib.check(self._L.sr_set_loss(self._ctx, self.LOSSES[kind], e))

    @property
    def loss(self):
        """(kind, eps) as sr_get_loss reports them: eps is the last one set with "charbonnier" (1e-3 on a fresh engine)."""
        kind, eps = C.c_int(), C.c_float()
        _lib.check(self._L.sr_get_loss(self._ctx, C.byref(kind), C.byref(eps)))
        return {v: k for k, v in self.LOSSES.items()}[kind.value], float(eps.value)

    def check_domain(self):
        """sr_check_domain: after the stream of earlier *_dev calls has been synchronised, raises SrError(SR_E_DOMAIN) if one of them
        left the domain of "split_f16" (a non-finite value, or one of 65504 and beyond); the host-pointer calls recompute in f32 themselves."""
        _lib.check(self._L.sr_check_domain(self._ctx))

    def _out_hw(self, h, w):
        return (h // 3, w // 3) if self.graph == "downsample" else (self.factor * h, self.factor * w)

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.sr_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    # ---- the prologues the entry points share: a method adds its own arguments and its call ----
    @staticmethod
    def _host_batch(arr, dtype, channels=None):
        """A numpy image (H,W,C) or batch (n,H,W,C) -> (arr4d, squeeze, n, h, w, c): C-contiguous, of `dtype` (None: its own), with
        `channels` channels (None: any); squeeze: it was one image, and the result is returned as one."""
        arr = np.ascontiguousarray(arr, dtype=dtype)
        squeeze = arr.ndim == 3
        if squeeze:
            arr = arr[None]
        n, h, w, c = arr.shape
        if channels is not None and c != channels:
            raise ValueError(f"expected {channels} channels")
        return arr, squeeze, n, h, w, c

    @staticmethod
    def _host_out(out, n, oh, ow, channels, dtype):
        """The (n,oh,ow,channels) numpy result: a new array, or the caller's `out` (any shape of that many elements) checked and reshaped."""
        if out is None:
            return np.empty((n, max(oh, 0), max(ow, 0), channels), dtype=dtype)
        if out.dtype != dtype or out.size != n * oh * ow * channels or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {'u8' if dtype == np.uint8 else 'f32'} array of n*oh*ow*{channels} elements")
        return out.reshape(n, oh, ow, channels)

    @staticmethod
    def _dev_batch(x, dtype, channels=None):
        """A contiguous (n,H,W,C) tensor on a GPU, of numpy `dtype` and `channels` channels (None: any) -> (n, h, w, c)."""
        import torch
        assert x.is_cuda and x.dtype == getattr(torch, np.dtype(dtype).name) and x.is_contiguous() and x.dim() == 4
        assert channels is None or x.shape[-1] == channels
        return tuple(x.shape)

    @staticmethod
    def _dev_out(out, shape, dtype, device):
        """The caller's `out`, or a new tensor of that shape and numpy `dtype` on the device."""
        import torch
        return out if out is not None else torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=device)

    # ---- host-memory entry points (numpy in, numpy out) --------------------
    def upscale_f32(self, x: np.ndarray) -> np.ndarray:
        """(n,H,W,3) or (H,W,3) f32 in [0,1] -> (n,3H,3W,3) f32 pre-quantisation."""
        x, squeeze, n, h, w, _ = self._host_batch(x, np.float32, 3)
        out = self._host_out(None, n, *self._out_hw(h, w), 3, np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._L.sr_upscale_f32(self._ctx, x.ctypes.data_as(fp), n, h, w, out.ctypes.data_as(fp)), self._ctx)
        return out[0] if squeeze else out

    def upscale_rgba8(self, px: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """(n,H,W,3|4) or (H,W,3|4) u8 -> (n,3H,3W,4) u8 RGBA (alpha 255).  `out` may be a
        page-locked array from host_alloc (copies then overlap the kernels at PCIe rate)."""
        px, squeeze, n, h, w, c = self._host_batch(px, np.uint8)
        out = self._host_out(out, n, *self._out_hw(h, w), 4, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_upscale_rgba8(self._ctx, px.ctypes.data_as(u8p), c, n, h, w, out.ctypes.data_as(u8p)), self._ctx)
        return out[0] if squeeze else out

    # ---- self-ensemble: the network averaged over the flips and rotations `members` names (include/srhip.h sr_upscale_ensemble_*) ----
    @staticmethod
    def _members(members) -> int:
        """The mask as the unsigned the ABI takes; what does not fit one (negative, huge) is refused here as the library would."""
        m = int(members)
        if m < 0 or m > 0xFFFFFFFF:
            raise _lib.SrError(_lib.SR_E_INVALID, f"members {members}")
        return m

    def upscale_ensemble_f32(self, x: np.ndarray, members: int = _lib.SR_ENSEMBLE_ALL) -> np.ndarray:
        """upscale_f32 averaged over the members of the mask (bit k: flip / rotation k; 0xFF all 8, 0x0F the 4 flips, 0x03 identity and
        the column flip): (n,H,W,3) or (H,W,3) f32 -> (n,fH,fW,3) f32."""
        x, squeeze, n, h, w, _ = self._host_batch(x, np.float32, 3)
        out = self._host_out(None, n, self.factor * h, self.factor * w, 3, np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._L.sr_upscale_ensemble_f32(self._ctx, x.ctypes.data_as(fp), n, h, w, out.ctypes.data_as(fp), self._members(members)),
                   self._ctx)
        return out[0] if squeeze else out

    def upscale_ensemble_rgba8(self, px: np.ndarray, members: int = _lib.SR_ENSEMBLE_ALL, out: np.ndarray = None) -> np.ndarray:
        """upscale_rgba8 averaged over the members of the mask, quantised once at the end: (n,H,W,3|4) or (H,W,3|4) u8 -> (n,fH,fW,4) u8."""
        px, squeeze, n, h, w, c = self._host_batch(px, np.uint8)
        out = self._host_out(out, n, self.factor * h, self.factor * w, 4, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_upscale_ensemble_rgba8(self._ctx, px.ctypes.data_as(u8p), c, n, h, w, out.ctypes.data_as(u8p),
                                                     self._members(members)), self._ctx)
        return out[0] if squeeze else out

    def reserve(self, n: int, h: int, w: int, io: str = "rgba8", channels: int = 3):
        """Allocate and warm everything upscale_rgba8 / upscale_f32 of that shape needs (sr_reserve_*): optional."""
        if io == "rgba8":
            _lib.check(self._L.sr_reserve_rgba8(self._ctx, channels, n, h, w), self._ctx)
        elif io == "f32":
            _lib.check(self._L.sr_reserve_f32(self._ctx, n, h, w), self._ctx)
        else:
            raise ValueError("io must be 'rgba8' or 'f32'")

    # ---- device-memory entry points (torch tensors on this GPU) ------------
    @staticmethod
    def _stream_ptr(stream=None, device=None):
        """The stream to launch on: the caller's, else torch's current stream OF THE TENSOR'S DEVICE (not of whatever device
        happens to be current in this thread: a process that drives several GPUs may be elsewhere)."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(device)
        return C.c_void_p(s.cuda_stream)

    def upscale_f32_dev(self, x, out=None, stream=None):
        n, h, w, _ = self._dev_batch(x, np.float32, 3)
        out = self._dev_out(out, (n,) + self._out_hw(h, w) + (3,), np.float32, x.device)
        _lib.check(self._L.sr_upscale_f32_dev(self._ctx, C.c_void_p(x.data_ptr()), n, h, w,
                                              C.c_void_p(out.data_ptr()), self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def upscale_rgba8_dev(self, px, out=None, stream=None):
        n, h, w, c = self._dev_batch(px, np.uint8)
        out = self._dev_out(out, (n,) + self._out_hw(h, w) + (4,), np.uint8, px.device)
        _lib.check(self._L.sr_upscale_rgba8_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w,
                                                C.c_void_p(out.data_ptr()), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    def upscale_ensemble_f32_dev(self, x, members: int = _lib.SR_ENSEMBLE_ALL, out=None, stream=None):
        n, h, w, _ = self._dev_batch(x, np.float32, 3)
        out = self._dev_out(out, (n, self.factor * h, self.factor * w, 3), np.float32, x.device)
        _lib.check(self._L.sr_upscale_ensemble_f32_dev(self._ctx, C.c_void_p(x.data_ptr()), n, h, w, C.c_void_p(out.data_ptr()),
                                                       self._members(members), self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def upscale_ensemble_rgba8_dev(self, px, members: int = _lib.SR_ENSEMBLE_ALL, out=None, stream=None):
        n, h, w, c = self._dev_batch(px, np.uint8)
        out = self._dev_out(out, (n, self.factor * h, self.factor * w, 4), np.uint8, px.device)
        _lib.check(self._L.sr_upscale_ensemble_rgba8_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w, C.c_void_p(out.data_ptr()),
                                                         self._members(members), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    # ---- transparency: colours bled under the transparent pixels, the alpha channel interpolated (include/srhip.h "Transparency") ----
    def _rgba_dev(self, px):
        """An (n,H,W,4) or (H,W,4) u8 image as a contiguous 4-d tensor on the GPU: a numpy array is uploaded, a tensor taken as it is."""
        import torch
        numpy_in = not torch.is_tensor(px)
        if numpy_in:
            px = torch.from_numpy(np.ascontiguousarray(px, dtype=np.uint8)).to(f"cuda:{self.device}")
        squeeze = px.dim() == 3
        if squeeze:
            px = px[None]
        assert px.is_cuda and px.dtype == torch.uint8 and px.is_contiguous() and px.dim() == 4 and px.shape[-1] == 4
        return px, squeeze, numpy_in

    @staticmethod
    def _rgba_result(out, squeeze, numpy_in):
        out = out[0] if squeeze else out
        return out.cpu().numpy() if numpy_in else out

    def bleed(self, img_rgba, radius: int = _lib.SR_ALPHA_BLEED_DEFAULT, out=None, stream=None):
        """sr_bleed_rgba8_dev: the colours of the pixels with alpha > 0 spread `radius` pixels (0..16) under the transparent ones, alpha
        untouched.  (n,H,W,4) or (H,W,4) u8, a tensor on this GPU (4-byte aligned) or a numpy array; the result is of the same kind."""
        import torch
        px, squeeze, numpy_in = self._rgba_dev(img_rgba)
        n, h, w, _ = px.shape
        if out is None:
            out = torch.empty_like(px)
        _lib.check(self._L.sr_bleed_rgba8_dev(self._ctx, C.c_void_p(px.data_ptr()), n, h, w, int(radius), C.c_void_p(out.data_ptr()),
                                              self._stream_ptr(stream, px.device)), self._ctx)
        return self._rgba_result(out, squeeze, numpy_in)

    def merge_alpha(self, lr_rgba, out_rgba, stream=None):
        """sr_merge_alpha_rgba8_dev: the alpha of lr_rgba (n,H,W,4), interpolated to (n,fH,fW), replaces byte 3 of every pixel of out_rgba
        IN PLACE when that is a tensor on this GPU; a numpy out_rgba is copied, and the merged copy returned."""
        import torch
        lr, squeeze, _ = self._rgba_dev(lr_rgba)
        out, _, numpy_out = self._rgba_dev(out_rgba)
        n, h, w, _ = lr.shape
        assert tuple(out.shape) == (n, self.factor * h, self.factor * w, 4) and out.device == lr.device
        _lib.check(self._L.sr_merge_alpha_rgba8_dev(self._ctx, C.c_void_p(lr.data_ptr()), n, h, w, C.c_void_p(out.data_ptr()),
                                                    self._stream_ptr(stream, lr.device)), self._ctx)
        return self._rgba_result(out, squeeze, numpy_out)

    def upscale_rgba8_alpha(self, img_rgba: np.ndarray, bleed: int = _lib.SR_ALPHA_BLEED_DEFAULT, members: int = 1, out: np.ndarray = None) -> np.ndarray:
        """upscale_rgba8 (members == 1) or upscale_ensemble_rgba8 (any other mask) that keeps transparency: (n,H,W,4) or (H,W,4) u8 ->
        (n,fH,fW,4) u8 whose RGB is the network's output on the image bled by `bleed` pixels and whose alpha is the input's, interpolated."""
        px, squeeze, n, h, w, _ = self._host_batch(img_rgba, np.uint8, 4)
        out = self._host_out(out, n, *self._out_hw(h, w), 4, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_upscale_rgba8_alpha(self._ctx, px.ctypes.data_as(u8p), n, h, w, out.ctypes.data_as(u8p), int(bleed),
                                                  self._members(members)), self._ctx)
        return out[0] if squeeze else out

    def upscale_rgba8_alpha_dev(self, px, bleed: int = _lib.SR_ALPHA_BLEED_DEFAULT, members: int = 1, out=None, stream=None):
        n, h, w, _ = self._dev_batch(px, np.uint8, 4)
        out = self._dev_out(out, (n,) + self._out_hw(h, w) + (4,), np.uint8, px.device)
        _lib.check(self._L.sr_upscale_rgba8_alpha_dev(self._ctx, C.c_void_p(px.data_ptr()), n, h, w, C.c_void_p(out.data_ptr()), int(bleed),
                                                      self._members(members), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    # ---- borders: the image continued by wrap / replicate / mirror, upscaled and cut back (include/srhip.h "Borders") ----
    BORDERS = {"wrap": _lib.SR_BORDER_WRAP, "replicate": _lib.SR_BORDER_REPLICATE, "mirror": _lib.SR_BORDER_MIRROR}

    @classmethod
    def _border_mode(cls, mode) -> int:
        """The mode by name; an integer passes as it is (the library refuses one it does not know)."""
        if isinstance(mode, str):
            if mode not in cls.BORDERS:
                raise ValueError(f"mode must be one of {sorted(cls.BORDERS)}")
            return cls.BORDERS[mode]
        return int(mode)

    @staticmethod
    def _pixels_dev(x):
        """(n,H,W,4) u8 or (n,H,W,3) f32, a contiguous tensor on the GPU -> (n, h, w, is_f32)."""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 4
        f32 = x.dtype == torch.float32
        assert (f32 and x.shape[-1] == 3) or (x.dtype == torch.uint8 and x.shape[-1] == 4)
        n, h, w, _ = x.shape
        return n, h, w, f32

    def pad(self, x, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, out=None, stream=None):
        """sr_pad_*_dev: (n,H,W,4) u8 or (n,H,W,3) f32 on this GPU -> (n,H+2p,W+2p,C), continued under `mode` by `pad` pixels (0..32)."""
        import torch
        n, h, w, f32 = self._pixels_dev(x)
        p = int(pad)
        if out is None:
            out = torch.empty((n, h + 2 * max(p, 0), w + 2 * max(p, 0), x.shape[-1]), dtype=x.dtype, device=x.device)
        fn = self._L.sr_pad_f32_dev if f32 else self._L.sr_pad_rgba8_dev
        _lib.check(fn(self._ctx, C.c_void_p(x.data_ptr()), n, h, w, self._border_mode(mode), p, C.c_void_p(out.data_ptr()),
                      self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def crop(self, x, y0: int, x0: int, ch: int, cw: int, out=None, stream=None):
        """sr_crop_*_dev: the ch x cw window at (y0, x0) of (n,H,W,4) u8 or (n,H,W,3) f32 on this GPU, as a contiguous (n,ch,cw,C) tensor."""
        import torch
        n, h, w, f32 = self._pixels_dev(x)
        if out is None:
            out = torch.empty((n, max(int(ch), 0), max(int(cw), 0), x.shape[-1]), dtype=x.dtype, device=x.device)
        fn = self._L.sr_crop_f32_dev if f32 else self._L.sr_crop_rgba8_dev
        _lib.check(fn(self._ctx, C.c_void_p(x.data_ptr()), n, h, w, int(y0), int(x0), int(ch), int(cw), C.c_void_p(out.data_ptr()),
                      self._stream_ptr(stream, x.device)), self._ctx)
        return out

    @staticmethod
    def _bleed_arg(bleed) -> int:
        return -1 if bleed is None else int(bleed)

    def upscale_rgba8_border(self, img_rgba: np.ndarray, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1, bleed=None,
                             out: np.ndarray = None) -> np.ndarray:
        """upscale_rgba8 (members == 1) or upscale_ensemble_rgba8 (any other mask) of the image continued under `mode`: (n,H,W,4) or
        (H,W,4) u8 -> (n,fH,fW,4) u8.  bleed: None for opaque output, 0..16 to keep transparency as upscale_rgba8_alpha does."""
        px, squeeze, n, h, w, _ = self._host_batch(img_rgba, np.uint8, 4)
        out = self._host_out(out, n, *self._out_hw(h, w), 4, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_upscale_rgba8_border(self._ctx, px.ctypes.data_as(u8p), n, h, w, out.ctypes.data_as(u8p), self._border_mode(mode),
                                                   int(pad), self._members(members), self._bleed_arg(bleed)), self._ctx)
        return out[0] if squeeze else out

    def upscale_f32_border(self, x: np.ndarray, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1) -> np.ndarray:
        """upscale_f32 (members == 1) or upscale_ensemble_f32 of the image continued under `mode`: (n,H,W,3) or (H,W,3) f32 -> (n,fH,fW,3)."""
        x, squeeze, n, h, w, _ = self._host_batch(x, np.float32, 3)
        out = self._host_out(None, n, *self._out_hw(h, w), 3, np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._L.sr_upscale_f32_border(self._ctx, x.ctypes.data_as(fp), n, h, w, out.ctypes.data_as(fp), self._border_mode(mode),
                                                 int(pad), self._members(members)), self._ctx)
        return out[0] if squeeze else out

    def upscale_rgba8_border_dev(self, px, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1, bleed=None, out=None,
                                 stream=None):
        n, h, w, _ = self._dev_batch(px, np.uint8, 4)
        out = self._dev_out(out, (n,) + self._out_hw(h, w) + (4,), np.uint8, px.device)
        _lib.check(self._L.sr_upscale_rgba8_border_dev(self._ctx, C.c_void_p(px.data_ptr()), n, h, w, C.c_void_p(out.data_ptr()),
                                                       self._border_mode(mode), int(pad), self._members(members), self._bleed_arg(bleed),
                                                       self._stream_ptr(stream, px.device)), self._ctx)
        return out

    def upscale_f32_border_dev(self, x, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1, out=None, stream=None):
        n, h, w, _ = self._dev_batch(x, np.float32, 3)
        out = self._dev_out(out, (n,) + self._out_hw(h, w) + (3,), np.float32, x.device)
        _lib.check(self._L.sr_upscale_f32_border_dev(self._ctx, C.c_void_p(x.data_ptr()), n, h, w, C.c_void_p(out.data_ptr()),
                                                     self._border_mode(mode), int(pad), self._members(members),
                                                     self._stream_ptr(stream, x.device)), self._ctx)
        return out

    # ---- video: planar YCbCr frames laid out like a Y4M frame payload, of bytes (include/srhip.h "Video") or of 9..16-bit samples in
    # uint16 (include/srhip.h "Deep video").  One set of helpers: `tag` is "yuv" or "yuv16", the word the library's symbols differ in ----
    @staticmethod
    def _yuv_kind(tag, fmt, h, w):
        """(numpy sample type, the torch dtype of a new result, samples in a frame of h x w)."""
        import torch
        if tag == "yuv":
            return np.uint8, torch.uint8, yuv_frame_bytes(fmt, h, w)
        return np.uint16, torch.int16, yuv16_frame_bytes(fmt, h, w) // 2   # (int16 tensors hold the uint16 samples)

    def _yuv_frames(self, tag, frames, fmt, h, w):
        """Host frames as a C-contiguous (n, frame_samples) array of the sample type; squeeze: it was one frame (1-d)."""
        dtype, _, fs = self._yuv_kind(tag, fmt, h, w)
        a = np.ascontiguousarray(frames, dtype=dtype)
        squeeze = a.ndim == 1
        if fs == 0 or a.ndim not in (1, 2) or a.shape[-1] != fs:
            raise ValueError(f"expected frames of {fs} {'bytes' if tag == 'yuv' else 'samples'}")
        return (a[None] if squeeze else a), squeeze

    def _yuv_frames_dev(self, tag, frames, fmt, h, w):
        """A contiguous tensor of samples on the GPU (torch.uint8; deep: torch.uint16 or torch.int16), (n, frame_samples) or
        (frame_samples,): any sample offset within its allocation will do."""
        dtype, tdtype, fs = self._yuv_kind(tag, fmt, h, w)
        assert frames.is_cuda and frames.is_contiguous() and frames.dim() in (1, 2) and frames.shape[-1] == fs
        assert frames.dtype == tdtype if tag == "yuv" else frames.element_size() == 2
        return 1 if frames.dim() == 1 else frames.shape[0]

    def _yuv_out_dev(self, tag, out, fmt, n, h, w, device):
        """The caller's `out`, or a new (n, frame_samples) tensor for frames of h x w."""
        import torch
        dtype, tdtype, fs = self._yuv_kind(tag, fmt, h, w)
        if out is None:
            out = torch.empty((n, fs), dtype=tdtype, device=device)
        assert out.is_cuda and out.element_size() == np.dtype(dtype).itemsize and out.is_contiguous() and out.numel() == n * fs
        return out

    def _yuv_to_rgb_dev(self, tag, frames, fmt, h, w, out, stream):
        n = self._yuv_frames_dev(tag, frames, fmt, h, w)
        out = self._dev_out(out, (n, h, w, 3), np.float32, frames.device)
        _lib.check(getattr(self._L, f"sr_{tag}_to_rgb_dev")(self._ctx, C.c_void_p(frames.data_ptr()), C.byref(fmt), n, h, w, C.c_void_p(out.data_ptr()),
                                                            self._stream_ptr(stream, frames.device)), self._ctx)
        return out

    def _rgb_to_yuv_dev(self, tag, x, fmt, out, stream):
        n, h, w, _ = self._dev_batch(x, np.float32, 3)
        out = self._yuv_out_dev(tag, out, fmt, n, h, w, x.device)
        _lib.check(getattr(self._L, f"sr_rgb_to_{tag}_dev")(self._ctx, C.c_void_p(x.data_ptr()), C.byref(fmt), n, h, w, C.c_void_p(out.data_ptr()),
                                                            self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def _upscale_yuv_dev(self, tag, frames, fmt, h, w, members, out, stream):
        n = self._yuv_frames_dev(tag, frames, fmt, h, w)
        out = self._yuv_out_dev(tag, out, fmt, n, self.factor * h, self.factor * w, frames.device)
        _lib.check(getattr(self._L, f"sr_upscale_{tag}_dev")(self._ctx, C.c_void_p(frames.data_ptr()), C.byref(fmt), n, h, w, C.c_void_p(out.data_ptr()),
                                                             self._members(members), self._stream_ptr(stream, frames.device)), self._ctx)
        return out

    def _yuv_to_rgb(self, tag, frames, fmt, h, w):
        import torch
        a, squeeze = self._yuv_frames(tag, frames, fmt, h, w)
        dev = torch.from_numpy(a if tag == "yuv" else a.view(np.int16)).to(f"cuda:{self.device}")
        out = self._yuv_to_rgb_dev(tag, dev, fmt, h, w, None, None)
        torch.cuda.synchronize(out.device)
        out = out.cpu().numpy()
        return out[0] if squeeze else out

    def _rgb_to_yuv(self, tag, x, fmt):
        import torch
        x, squeeze, _, h, w, _ = self._host_batch(x, np.float32, 3)
        out = self._rgb_to_yuv_dev(tag, torch.from_numpy(x).to(f"cuda:{self.device}"), fmt, None, None)
        torch.cuda.synchronize(out.device)
        out = out.cpu().numpy().view(self._yuv_kind(tag, fmt, h, w)[0])
        return out[0] if squeeze else out

    def _upscale_yuv(self, tag, frames, fmt, h, w, members, out):
        a, squeeze = self._yuv_frames(tag, frames, fmt, h, w)
        dtype, _, os_ = self._yuv_kind(tag, fmt, self.factor * h, self.factor * w)
        n = a.shape[0]
        if out is None:
            out = np.empty((n, os_), dtype=dtype)
        elif out.dtype != dtype or out.size != n * os_ or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {'u8' if tag == 'yuv' else 'u16'} array of {n * os_} {'bytes' if tag == 'yuv' else 'samples'}")
        ptr = C.POINTER(C.c_uint8 if tag == "yuv" else C.c_uint16)
        _lib.check(getattr(self._L, f"sr_upscale_{tag}")(self._ctx, a.ctypes.data_as(ptr), C.byref(fmt), n, h, w, out.ctypes.data_as(ptr),
                                                         self._members(members)), self._ctx)
        out = out.reshape(n, os_)
        return out[0] if squeeze else out

    def yuv_to_rgb_dev(self, frames, fmt, h: int, w: int, out=None, stream=None):
        """sr_yuv_to_rgb_dev: (n, frame_bytes) u8 on this GPU -> (n,h,w,3) f32 RGB in [0, 1], the network's input."""
        return self._yuv_to_rgb_dev("yuv", frames, fmt, h, w, out, stream)

    def rgb_to_yuv_dev(self, x, fmt, out=None, stream=None):
        """sr_rgb_to_yuv_dev: (n,h,w,3) f32 RGB on this GPU (any finite values: clamped; NaN counts as 0) -> (n, frame_bytes) u8."""
        return self._rgb_to_yuv_dev("yuv", x, fmt, out, stream)

    def upscale_yuv_dev(self, frames, fmt, h: int, w: int, members: int = 1, out=None, stream=None):
        """sr_upscale_yuv_dev: (n, frame_bytes) u8 frames of h x w on this GPU -> (n, frame_bytes of fh x fw) in the same format."""
        return self._upscale_yuv_dev("yuv", frames, fmt, h, w, members, out, stream)

    def rows_differ_dev(self, a, b, rows: int, row_bytes: int, out=None, stream=None):
        """sr_rows_differ_dev: two contiguous u8 tensors on this GPU, each holding rows x row_bytes bytes from its first element (views at
        any byte offset will do) -> (rows,) int32 flags, 1 where the row differs.  The frame stream's row reuse compares with it."""
        import torch
        assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.uint8 and a.is_contiguous() and b.is_contiguous()
        assert a.numel() >= rows * row_bytes and b.numel() >= rows * row_bytes
        out = self._dev_out(out, (rows,), np.int32, a.device)
        _lib.check(self._L.sr_rows_differ_dev(self._ctx, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), int(rows), int(row_bytes),
                                              C.c_void_p(out.data_ptr()), self._stream_ptr(stream, a.device)), self._ctx)
        return out

    def yuv_to_rgb(self, frames: np.ndarray, fmt, h: int, w: int) -> np.ndarray:
        """yuv_to_rgb_dev on host frames: (n, frame_bytes) or (frame_bytes,) u8 -> (n,h,w,3) or (h,w,3) f32."""
        return self._yuv_to_rgb("yuv", frames, fmt, h, w)

    def rgb_to_yuv(self, x: np.ndarray, fmt) -> np.ndarray:
        """rgb_to_yuv_dev on a host image: (n,h,w,3) or (h,w,3) f32 -> (n, frame_bytes) or (frame_bytes,) u8."""
        return self._rgb_to_yuv("yuv", x, fmt)

    def upscale_yuv(self, frames: np.ndarray, fmt, h: int, w: int, members: int = 1, out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_yuv: (n, frame_bytes) or (frame_bytes,) u8 frames of h x w -> the frames of fh x fw in the same format: colour
        conversion and chroma resampling on the GPU, the network's f32 output quantised once, straight to YCbCr."""
        return self._upscale_yuv("yuv", frames, fmt, h, w, members, out)

    def yuv16_to_rgb_dev(self, frames, fmt, h: int, w: int, out=None, stream=None):
        """sr_yuv16_to_rgb_dev: (n, frame_samples) 16-bit samples on this GPU -> (n,h,w,3) f32 RGB in [0, 1], the network's input."""
        return self._yuv_to_rgb_dev("yuv16", frames, fmt, h, w, out, stream)

    def rgb_to_yuv16_dev(self, x, fmt, out=None, stream=None):
        """sr_rgb_to_yuv16_dev: (n,h,w,3) f32 RGB on this GPU (any values: clamped; NaN counts as 0) -> (n, frame_samples) int16 tensor
        holding the uint16 samples (view it as torch.uint16, or numpy .view(np.uint16))."""
        return self._rgb_to_yuv_dev("yuv16", x, fmt, out, stream)

    def upscale_yuv16_dev(self, frames, fmt, h: int, w: int, members: int = 1, out=None, stream=None):
        """sr_upscale_yuv16_dev: (n, frame_samples) frames of h x w on this GPU -> (n, frame_samples of fh x fw) in the same format (int16
        tensor holding the uint16 samples unless `out` is given)."""
        return self._upscale_yuv_dev("yuv16", frames, fmt, h, w, members, out, stream)

    def yuv16_to_rgb(self, frames: np.ndarray, fmt, h: int, w: int) -> np.ndarray:
        """yuv16_to_rgb_dev on host frames: (n, frame_samples) or (frame_samples,) u16 -> (n,h,w,3) or (h,w,3) f32."""
        return self._yuv_to_rgb("yuv16", frames, fmt, h, w)

    def rgb_to_yuv16(self, x: np.ndarray, fmt) -> np.ndarray:
        """rgb_to_yuv16_dev on a host image: (n,h,w,3) or (h,w,3) f32 -> (n, frame_samples) or (frame_samples,) u16."""
        return self._rgb_to_yuv("yuv16", x, fmt)

    def upscale_yuv16(self, frames: np.ndarray, fmt, h: int, w: int, members: int = 1, out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_yuv16: (n, frame_samples) or (frame_samples,) u16 frames of h x w -> the frames of fh x fw in the same format."""
        return self._upscale_yuv("yuv16", frames, fmt, h, w, members, out)

    # ---- deep colour: 16-bit samples in and out (include/srhip.h "Deep colour") ----
    @staticmethod
    def _u16_host(px):
        """A numpy uint16 image (H,W), (H,W,C) or batch (n,H,W,C) -> (arr4d, squeeze, grey2d, n, h, w, c), C-contiguous."""
        px = np.ascontiguousarray(px, dtype=np.uint16)
        grey2d = px.ndim == 2
        if grey2d:
            px = px[:, :, None]
        squeeze = px.ndim == 3
        if squeeze:
            px = px[None]
        if px.ndim != 4 or not 1 <= px.shape[-1] <= 4:
            raise ValueError("expected uint16 samples shaped (h,w), (h,w,C) or (n,h,w,C) with C in 1..4")
        return (px, squeeze, grey2d) + tuple(px.shape)

    @staticmethod
    def _u16_out_channels(channels, in_channels, out=None):
        """The result's channel count: the caller's, else `out`'s, else grey for grey (1 or 2 channels in) and RGB otherwise."""
        if channels is None:
            channels = out.shape[-1] if out is not None and out.ndim >= 3 else (1 if in_channels <= 2 else 3)
        return int(channels)

    def _u16_result(self, out, n, oh, ow, oc):
        if out is None:
            return np.empty((n, max(oh, 0), max(ow, 0), max(oc, 1)), dtype=np.uint16)
        if out.dtype != np.uint16 or out.size != n * oh * ow * oc or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous uint16 array of n*oh*ow*{oc} samples")
        return out.reshape(n, oh, ow, oc)

    @staticmethod
    def _u16_shaped(out, squeeze, grey2d):
        out = out[0] if squeeze else out
        return out[:, :, 0] if grey2d and out.shape[-1] == 1 else out

    @staticmethod
    def _u16_dev(px):
        """A contiguous (n,H,W,C) torch.uint16 tensor on a GPU, C in 1..4 -> (n, h, w, c)."""
        import torch
        assert px.is_cuda and px.dtype == torch.uint16 and px.is_contiguous() and px.dim() == 4 and 1 <= px.shape[-1] <= 4
        return tuple(px.shape)

    def _u16_dev_out(self, out, n, oh, ow, oc, device):
        import torch
        if out is None and oh >= 1 and ow >= 1 and oc >= 1:
            out = torch.empty((n, oh, ow, oc), dtype=torch.uint16, device=device)
        return out, C.c_void_p(out.data_ptr() if out is not None else None)

    def u16_to_f32_dev(self, px, out=None, stream=None):
        """sr_u16_to_f32_dev: (n,h,w,C) torch.uint16 on this GPU, C in 1..4 -> (n,h,w,3) f32, sample / 65535 (grey copied to R = G = B,
        alpha dropped): the network's input."""
        n, h, w, c = self._u16_dev(px)
        out = self._dev_out(out, (n, h, w, 3), np.float32, px.device)
        _lib.check(self._L.sr_u16_to_f32_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w, C.c_void_p(out.data_ptr()),
                                             self._stream_ptr(stream, px.device)), self._ctx)
        return out

    def f32_to_u16_dev(self, x, channels: int = 3, out=None, stream=None):
        """sr_f32_to_u16_dev: (n,h,w,3) f32 on this GPU (any values: clamped; NaN counts as 0) -> (n,h,w,channels) torch.uint16,
        floor(65535 v + 0.5); channels 3 RGB, 4 RGBA with alpha 65535, 1 the grey mean."""
        n, h, w, _ = self._dev_batch(x, np.float32, 3)
        out, ptr = self._u16_dev_out(out, n, h, w, int(channels), x.device)
        _lib.check(self._L.sr_f32_to_u16_dev(self._ctx, C.c_void_p(x.data_ptr()), n, h, w, ptr, int(channels),
                                             self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def upscale_u16(self, px: np.ndarray, channels=None, members: int = 1, out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_u16: uint16 samples (n,h,w,C), (h,w,C) or (h,w) -> (n,fh,fw,channels) in the same arrangement, the network's f32
        output quantised once to 65536 levels.  channels: 1, 3 or 4 (default: grey for grey, RGB otherwise)."""
        px, squeeze, grey2d, n, h, w, c = self._u16_host(px)
        oc = self._u16_out_channels(channels, c, out)
        out = self._u16_result(out, n, *self._out_hw(h, w), oc)
        p = C.POINTER(C.c_uint16)
        _lib.check(self._L.sr_upscale_u16(self._ctx, px.ctypes.data_as(p), c, n, h, w, out.ctypes.data_as(p), oc, self._members(members)),
                   self._ctx)
        return self._u16_shaped(out, squeeze, grey2d)

    def upscale_u16_dev(self, px, channels=None, members: int = 1, out=None, stream=None):
        """sr_upscale_u16_dev: (n,h,w,C) torch.uint16 on this GPU -> (n,fh,fw,channels) torch.uint16."""
        n, h, w, c = self._u16_dev(px)
        oc = self._u16_out_channels(channels, c, out)
        out, ptr = self._u16_dev_out(out, n, *self._out_hw(h, w), oc, px.device)
        _lib.check(self._L.sr_upscale_u16_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w, ptr, oc, self._members(members),
                                              self._stream_ptr(stream, px.device)), self._ctx)
        return out

    def upscale_u16_border(self, px: np.ndarray, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1, channels=None,
                           out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_u16_border: upscale_u16 of the image continued under `mode` (upscale_f32_border between the two conversions)."""
        px, squeeze, grey2d, n, h, w, c = self._u16_host(px)
        oc = self._u16_out_channels(channels, c, out)
        out = self._u16_result(out, n, *self._out_hw(h, w), oc)
        p = C.POINTER(C.c_uint16)
        _lib.check(self._L.sr_upscale_u16_border(self._ctx, px.ctypes.data_as(p), c, n, h, w, out.ctypes.data_as(p), oc, self._border_mode(mode),
                                                 int(pad), self._members(members)), self._ctx)
        return self._u16_shaped(out, squeeze, grey2d)

    def upscale_u16_border_dev(self, px, mode="wrap", pad: int = _lib.SR_BORDER_PAD_DEFAULT, members: int = 1, channels=None, out=None,
                               stream=None):
        n, h, w, c = self._u16_dev(px)
        oc = self._u16_out_channels(channels, c, out)
        out, ptr = self._u16_dev_out(out, n, *self._out_hw(h, w), oc, px.device)
        _lib.check(self._L.sr_upscale_u16_border_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w, ptr, oc, self._border_mode(mode), int(pad),
                                                     self._members(members), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    def upscale_u16_sized(self, px: np.ndarray, size, filter="lanczos3", srgb_space=False, members: int = 1, channels=None,
                          out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_u16_sized: upscale_u16 to size = (oh, ow), the network's f32 output resampled on the device and quantised once."""
        px, squeeze, grey2d, n, h, w, c = self._u16_host(px)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        oc = self._u16_out_channels(channels, c, out)
        out = self._u16_result(out, n, oh, ow, oc)
        p = C.POINTER(C.c_uint16)
        _lib.check(self._L.sr_upscale_u16_sized(self._ctx, px.ctypes.data_as(p), c, n, h, w, out.ctypes.data_as(p), oc, oh, ow, flt, flags,
                                                self._members(members)), self._ctx)
        return self._u16_shaped(out, squeeze, grey2d)

    def upscale_u16_sized_dev(self, px, size, filter="lanczos3", srgb_space=False, members: int = 1, channels=None, out=None, stream=None):
        n, h, w, c = self._u16_dev(px)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        oc = self._u16_out_channels(channels, c, out)
        out, ptr = self._u16_dev_out(out, n, oh, ow, oc, px.device)
        _lib.check(self._L.sr_upscale_u16_sized_dev(self._ctx, C.c_void_p(px.data_ptr()), c, n, h, w, ptr, oc, oh, ow, flt, flags,
                                                    self._members(members), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    # ---- resampling to any size: a separable resampler in Pillow's convention, on the device (include/srhip.h "Resampling to any size") ----
    FILTERS = {"box": _lib.SR_FILTER_BOX, "triangle": _lib.SR_FILTER_TRIANGLE, "catrom": _lib.SR_FILTER_CATROM,
               "lanczos3": _lib.SR_FILTER_LANCZOS3}
    PIXELS = {"rgba8": _lib.SR_PIXELS_RGBA8, "f32": _lib.SR_PIXELS_F32}

    @classmethod
    def _resize_args(cls, size, filter, srgb_space):
        """(oh, ow), the filter's number (a name of FILTERS, or the number itself) and the flags word of the sr_resize_* calls."""
        oh, ow = (int(v) for v in size)
        return oh, ow, cls.FILTERS[filter] if isinstance(filter, str) else int(filter), _lib.SR_RESIZE_SRGB_SPACE if srgb_space else 0

    def resize_dev(self, x, size, out_pixels=None, filter="lanczos3", srgb_space=False, out=None, stream=None):
        """sr_resize_dev: (n,H,W,4) u8 RGBA or (n,H,W,3) f32 on this GPU -> (n,oh,ow,4) u8 (alpha 255) or (n,oh,ow,3) f32, size = (oh, ow).
        out_pixels: "rgba8" or "f32" (default: the input's kind, or `out`'s)."""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dim() == 4
        in_u8 = x.dtype == torch.uint8
        assert (in_u8 and x.shape[-1] == 4) or (x.dtype == torch.float32 and x.shape[-1] == 3)
        n, h, w, _ = x.shape
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        if out_pixels is None:
            out_pixels = ("rgba8" if out.dtype == torch.uint8 else "f32") if out is not None else ("rgba8" if in_u8 else "f32")
        out_u8 = self.PIXELS[out_pixels] == _lib.SR_PIXELS_RGBA8
        if out is None and oh >= 1 and ow >= 1:
            out = torch.empty((n, oh, ow, 4 if out_u8 else 3), dtype=torch.uint8 if out_u8 else torch.float32, device=x.device)
        _lib.check(self._L.sr_resize_dev(self._ctx, C.c_void_p(x.data_ptr()), _lib.SR_PIXELS_RGBA8 if in_u8 else _lib.SR_PIXELS_F32, n, h, w,
                                         C.c_void_p(out.data_ptr() if out is not None else None), self.PIXELS[out_pixels], oh, ow, flt, flags,
                                         self._stream_ptr(stream, x.device)), self._ctx)
        return out

    def resize(self, img, size, filter="lanczos3", srgb_space=False, out=None):
        """(n,H,W,4) or (H,W,4) u8 RGBA -> u8 RGBA (sr_resize_rgba8), or (n,H,W,3) or (H,W,3) f32 -> f32 (through sr_resize_dev), numpy in
        and out, resampled to size = (oh, ow)."""
        img, squeeze, n, h, w, c = self._host_batch(img, None)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        if img.dtype == np.uint8:
            if c != 4:
                raise ValueError("expected 4 channels")
            out = self._host_out(out, n, oh, ow, 4, np.uint8)
            u8p = C.POINTER(C.c_uint8)
            _lib.check(self._L.sr_resize_rgba8(self._ctx, img.ctypes.data_as(u8p), n, h, w, out.ctypes.data_as(u8p), oh, ow, flt, flags), self._ctx)
        else:
            import torch
            if img.dtype != np.float32 or c != 3:
                raise ValueError("expected u8 RGBA or f32 RGB")
            res = self.resize_dev(torch.from_numpy(img).to(f"cuda:{self.device}"), (oh, ow), "f32", flt, srgb_space).cpu().numpy()
            if out is not None:
                out = out.reshape(res.shape)
                out[...] = res
            else:
                out = res
        return out[0] if squeeze else out

    # ---- video at any size (include/srhip.h "Video at any size") ----
    def _yuv_host_out(self, tag, out, fmt, n, oh, ow):
        """The caller's `out`, or a new (n, frame_samples) array for frames of oh x ow (an invalid size: one sample, for the library to refuse)."""
        dtype, _, os_ = self._yuv_kind(tag, fmt, oh, ow) if oh >= 1 and ow >= 1 else (np.uint8 if tag == "yuv" else np.uint16, None, 0)
        if out is None:
            out = np.empty((n, max(os_, 1)), dtype=dtype)
        elif out.dtype != dtype or (os_ and out.size != n * os_) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous {'u8' if tag == 'yuv' else 'u16'} array of {n * os_} {'bytes' if tag == 'yuv' else 'samples'}")
        return out, os_, C.POINTER(C.c_uint8 if tag == "yuv" else C.c_uint16)

    def _resize_to_yuv(self, tag, x, fmt, size, filter, srgb_space, out):
        x, squeeze, n, h, w, _ = self._host_batch(x, np.float32, 3)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        out, os_, ptr = self._yuv_host_out(tag, out, fmt, n, oh, ow)
        _lib.check(getattr(self._L, f"sr_resize_to_{tag}")(self._ctx, C.c_void_p(x.ctypes.data), C.byref(fmt), n, h, w, out.ctypes.data_as(ptr),
                                                           oh, ow, flt, flags), self._ctx)
        out = out.reshape(n, os_)
        return out[0] if squeeze else out

    def _upscale_yuv_sized(self, tag, frames, fmt, h, w, size, filter, srgb_space, members, out):
        a, squeeze = self._yuv_frames(tag, frames, fmt, h, w)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        n = a.shape[0]
        out, os_, ptr = self._yuv_host_out(tag, out, fmt, n, oh, ow)
        _lib.check(getattr(self._L, f"sr_upscale_{tag}_sized")(self._ctx, a.ctypes.data_as(ptr), C.byref(fmt), n, h, w, out.ctypes.data_as(ptr),
                                                               oh, ow, flt, flags, self._members(members)), self._ctx)
        out = out.reshape(n, os_)
        return out[0] if squeeze else out

    def resize_to_yuv(self, x: np.ndarray, fmt, size, filter="lanczos3", srgb_space=False, out: np.ndarray = None) -> np.ndarray:
        """sr_resize_to_yuv: (n,h,w,3) or (h,w,3) f32 RGB -> (n, frame_bytes) or (frame_bytes,) u8 frames of size = (oh, ow): the bytes of
        resize (f32 -> f32) followed by rgb_to_yuv, without the f32 image in between."""
        return self._resize_to_yuv("yuv", x, fmt, size, filter, srgb_space, out)

    def resize_to_yuv16(self, x: np.ndarray, fmt, size, filter="lanczos3", srgb_space=False, out: np.ndarray = None) -> np.ndarray:
        """sr_resize_to_yuv16: resize_to_yuv to deep frames, (n, frame_samples) or (frame_samples,) u16."""
        return self._resize_to_yuv("yuv16", x, fmt, size, filter, srgb_space, out)

    def upscale_yuv_sized(self, frames: np.ndarray, fmt, h: int, w: int, size, filter="lanczos3", srgb_space=False, members: int = 1,
                          out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_yuv_sized: (n, frame_bytes) or (frame_bytes,) u8 frames of h x w -> the frames of size = (oh, ow) in the same format:
        the network's f32 output resampled on the GPU and quantised once, at the final size."""
        return self._upscale_yuv_sized("yuv", frames, fmt, h, w, size, filter, srgb_space, members, out)

    def upscale_yuv16_sized(self, frames: np.ndarray, fmt, h: int, w: int, size, filter="lanczos3", srgb_space=False, members: int = 1,
                            out: np.ndarray = None) -> np.ndarray:
        """sr_upscale_yuv16_sized: upscale_yuv_sized on deep frames, u16 in and out."""
        return self._upscale_yuv_sized("yuv16", frames, fmt, h, w, size, filter, srgb_space, members, out)

    def upscale_rgba8_sized(self, px: np.ndarray, size, filter="lanczos3", srgb_space=False, members: int = 1, out: np.ndarray = None) -> np.ndarray:
        """upscale_rgba8 (members == 1) or upscale_ensemble_rgba8 (any other mask) to size = (oh, ow): (n,H,W,4) or (H,W,4) u8 -> (n,oh,ow,4)
        u8, the network's f32 output resampled on the device and quantised once."""
        px, squeeze, n, h, w, _ = self._host_batch(px, np.uint8, 4)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        out = self._host_out(out, n, oh, ow, 4, np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_upscale_rgba8_sized(self._ctx, px.ctypes.data_as(u8p), n, h, w, out.ctypes.data_as(u8p), oh, ow, flt, flags,
                                                  self._members(members)), self._ctx)
        return out[0] if squeeze else out

    def upscale_rgba8_sized_dev(self, px, size, filter="lanczos3", srgb_space=False, members: int = 1, out=None, stream=None):
        n, h, w, _ = self._dev_batch(px, np.uint8, 4)
        oh, ow, flt, flags = self._resize_args(size, filter, srgb_space)
        if oh >= 1 and ow >= 1:  # (else a null pointer, which the library refuses)
            out = self._dev_out(out, (n, oh, ow, 4), np.uint8, px.device)
        _lib.check(self._L.sr_upscale_rgba8_sized_dev(self._ctx, C.c_void_p(px.data_ptr()), n, h, w,
                                                      C.c_void_p(out.data_ptr() if out is not None else None), oh, ow, flt, flags,
                                                      self._members(members), self._stream_ptr(stream, px.device)), self._ctx)
        return out

    # ---- degradation: blur, noise and a JPEG round trip of an HR frame, made on the device (include/srhip.h "Degradation") ----
    @staticmethod
    def _degrade_args(shape, factor, sigma, noise, quality, seed, window, member):
        f = int(factor)
        h, w = shape[:2]
        if window is None:
            window = (0, 0, h // f * f if f > 0 else 0, w // f * f if f > 0 else 0)
        y0, x0, fh, fw = (int(v) for v in window)
        return f, y0, x0, fh, fw, int(member), _lib.Degrade(float(sigma), float(noise), int(quality), int(seed) & (2 ** 64 - 1))

    def degrade(self, hr: np.ndarray, factor: int, sigma: float = 0.0, noise: float = 0.0, quality: int = 0, seed: int = 0, window=None,
                member: int = 0) -> np.ndarray:
        """(H,W,3|4) u8 -> the degraded LR frame, (frame_h / factor, frame_w / factor, 3) u8 (sr_degrade_rgba8): Gaussian blur of width
        sigma (HR pixels, linear light), the factor's pool, noise of that standard deviation (8-bit levels, stream `seed`), JPEG round trip
        at `quality` (0: none).  window: (y0, x0, frame_h, frame_w) in HR pixels, default the image cropped to a multiple of the factor;
        member: 0..7, the frame is T_k of the source window.  Any engine will do: no network runs."""
        hr = np.ascontiguousarray(hr)
        if hr.dtype != np.uint8 or hr.ndim != 3:
            raise ValueError("expected (H, W, 3|4) u8 pixels")
        f, y0, x0, fh, fw, k, g = self._degrade_args(hr.shape, factor, sigma, noise, quality, seed, window, member)
        out = np.empty((max(fh // f, 0) if f > 0 else 0, max(fw // f, 0) if f > 0 else 0, 3), dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_degrade_rgba8(self._ctx, hr.ctypes.data_as(u8p), hr.shape[2], hr.shape[0], hr.shape[1], f, y0, x0, fh, fw, k,
                                            C.byref(g), out.ctypes.data_as(u8p)), self._ctx)
        return out

    def degrade_dev(self, hr, factor: int, sigma: float = 0.0, noise: float = 0.0, quality: int = 0, seed: int = 0, window=None, member: int = 0,
                    out=None, stream=None):
        """degrade on a (H,W,3|4) u8 torch tensor of this engine's device -> a (frame_h / factor, frame_w / factor, 3) u8 tensor,
        asynchronous on the stream (sr_degrade_rgba8_dev).  hr and out may start at any byte."""
        import torch
        assert hr.is_cuda and hr.dtype == torch.uint8 and hr.is_contiguous() and hr.dim() == 3
        f, y0, x0, fh, fw, k, g = self._degrade_args(hr.shape, factor, sigma, noise, quality, seed, window, member)
        if out is None and f > 0 and fh >= f and fw >= f:
            out = torch.empty((fh // f, fw // f, 3), dtype=torch.uint8, device=hr.device)
        _lib.check(self._L.sr_degrade_rgba8_dev(self._ctx, C.c_void_p(hr.data_ptr()), hr.shape[2], hr.shape[0], hr.shape[1], f, y0, x0, fh, fw, k,
                                                C.byref(g), C.c_void_p(out.data_ptr() if out is not None else None),
                                                self._stream_ptr(stream, hr.device)), self._ctx)
        return out

    def upscale_band_f32_dev(self, x_ext, halo_top, halo_bot, out=None, stream=None):
        """x_ext: (h_ext,W,3) f32 rows = halo_top + band + halo_bot -> (3*band,3W,3)."""
        import torch
        assert x_ext.is_cuda and x_ext.dtype == torch.float32 and x_ext.is_contiguous() and x_ext.dim() == 3
        h_ext, w, _ = x_ext.shape
        hb = h_ext - halo_top - halo_bot
        if hb <= 0 or halo_top < 0 or halo_bot < 0:
            raise _lib.SrError(_lib.SR_E_INVALID)
        if out is None:
            out = torch.empty((self.factor * hb, self.factor * w, 3), dtype=torch.float32, device=x_ext.device)
        _lib.check(self._L.sr_upscale_band_f32_dev(self._ctx, C.c_void_p(x_ext.data_ptr()), h_ext, w, halo_top,
                                                   halo_bot, C.c_void_p(out.data_ptr()), self._stream_ptr(stream, x_ext.device)),
                   self._ctx)
        return out

    def upscale_band_rgba8_dev(self, px_ext, halo_top, halo_bot, out=None, stream=None):
        import torch
        assert px_ext.is_cuda and px_ext.dtype == torch.uint8 and px_ext.is_contiguous() and px_ext.dim() == 3
        h_ext, w, c = px_ext.shape
        hb = h_ext - halo_top - halo_bot
        if hb <= 0 or halo_top < 0 or halo_bot < 0:
            raise _lib.SrError(_lib.SR_E_INVALID)
        if out is None:
            out = torch.empty((self.factor * hb, self.factor * w, 4), dtype=torch.uint8, device=px_ext.device)
        _lib.check(self._L.sr_upscale_band_rgba8_dev(self._ctx, C.c_void_p(px_ext.data_ptr()), c, h_ext, w,
                                                     halo_top, halo_bot, C.c_void_p(out.data_ptr()),
                                                     self._stream_ptr(stream, px_ext.device)), self._ctx)
        return out

    # ---- sharded image: RCCL communicator inside libsrhip (include/srhip.h sr_comm_*) ----------
    @staticmethod
    def comm_unique_id() -> bytes:
        """128 opaque bytes from rank 0 (ncclGetUniqueId) that every rank passes to comm_init_rank."""
        buf = (C.c_uint8 * _lib.SR_COMM_ID_BYTES)()
        _lib.check(_lib.lib().sr_comm_unique_id(buf, _lib.SR_COMM_ID_BYTES))
        return bytes(buf)

    def comm_init_rank(self, uid: bytes, rank: int, nranks: int):
        """Join the band communicator as `rank` of `nranks` (collective; one process per GPU)."""
        buf = (C.c_uint8 * _lib.SR_COMM_ID_BYTES).from_buffer_copy(uid) if nranks > 1 else None
        _lib.check(self._L.sr_comm_init_rank(self._ctx, buf, _lib.SR_COMM_ID_BYTES if nranks > 1 else 0, rank, nranks), self._ctx)

    def comm_rank(self):
        r, n = C.c_int(), C.c_int()
        _lib.check(self._L.sr_comm_rank(self._ctx, C.byref(r), C.byref(n)))
        return r.value, n.value

    def last_comm_ms(self) -> float:
        v = C.c_double()
        _lib.check(self._L.sr_last_comm_ms(self._ctx, C.byref(v)))
        return v.value

    def last_comm_exposed_ms(self) -> float:
        """What of the last sharded call's halo exchange the band's stream had to wait for (sr_last_comm_exposed_ms)."""
        v = C.c_double()
        _lib.check(self._L.sr_last_comm_exposed_ms(self._ctx, C.byref(v)))
        return v.value

    def upscale_sharded_dev(self, band, out=None, stream=None):
        """This rank's band (rows, W, 3 f32 | 3-4 u8) of an image sharded in rank order: halo exchange over the
        context's RCCL communicator + band pass, asynchronous on the stream -> (3 rows, 3 W, 3 f32 | 4 u8)."""
        import torch
        assert band.is_cuda and band.is_contiguous() and band.dim() == 3
        hb, w, c = band.shape
        u8 = band.dtype == torch.uint8
        assert u8 or (band.dtype == torch.float32 and c == 3)
        if out is None:
            out = torch.empty((self.factor * hb, self.factor * w, 4 if u8 else 3), dtype=band.dtype, device=band.device)
        if u8:
            st = self._L.sr_upscale_sharded_rgba8_dev(self._ctx, C.c_void_p(band.data_ptr()), c, hb, w, C.c_void_p(out.data_ptr()),
                                                      self._stream_ptr(stream, band.device))
        else:
            st = self._L.sr_upscale_sharded_f32_dev(self._ctx, C.c_void_p(band.data_ptr()), hb, w, C.c_void_p(out.data_ptr()),
                                                    self._stream_ptr(stream, band.device))
        _lib.check(st, self._ctx)
        return out

    # ---- validation: the forward half of the training graph (reference main.rs:220-247, network.rs:88-102) ----
    def validation_error(self, hr: np.ndarray, linear_loss: bool = False, members=None):
        """HR image (H,W,3|4) u8 (img_to_data: byte / 255, alpha dropped) or (H,W,3) f32 -> (err_sum, n_elems): the squared error of
        sr_net(f)(LinearToSrgb(mean_fxf(SrgbToLinear(hr)))) against hr (of SrgbToLinear of both with linear_loss) over the top-left
        f*(H//f) x f*(W//f) crop, and the number of elements compared (sr_validation_error_*).  members: None, or the mask of a
        self-ensemble whose output is scored in the network's place (u8 images only; sr_pool_validation_error_ensemble_rgba8)."""
        hr = np.asarray(hr)
        if hr.ndim != 3:
            raise ValueError("expected one (H, W, C) image")
        h, w, c = hr.shape
        err, n = C.c_double(), C.c_size_t()
        if members is not None:
            if hr.dtype != np.uint8:
                raise ValueError("the ensemble form takes u8 pixels")
            hr = np.ascontiguousarray(hr)
            st = self._L.sr_pool_validation_error_ensemble_rgba8(self._ctx, hr.ctypes.data_as(C.POINTER(C.c_uint8)), c, h, w, int(bool(linear_loss)),
                                                            self._members(members), C.byref(err), C.byref(n))
        elif hr.dtype == np.uint8:
            hr = np.ascontiguousarray(hr)
            st = self._L.sr_validation_error_rgba8(self._ctx, hr.ctypes.data_as(C.POINTER(C.c_uint8)), c, h, w, int(bool(linear_loss)),
                                                   C.byref(err), C.byref(n))
        elif hr.dtype == np.float32:
            if c != 3:
                raise ValueError("an f32 HR image has 3 channels")
            hr = np.ascontiguousarray(hr)
            st = self._L.sr_validation_error_f32(self._ctx, hr.ctypes.data_as(C.POINTER(C.c_float)), h, w, int(bool(linear_loss)),
                                                 C.byref(err), C.byref(n))
        else:
            raise ValueError("expected u8 or f32 pixels")
        _lib.check(st, self._ctx)
        return err.value, n.value

    def validation_error_dev(self, hr, linear_loss: bool = False, out=None, stream=None):
        """(H,W,3|4) u8 torch tensor on this engine's device -> a float64 tensor of one element holding err_sum, asynchronous on the
        stream (sr_validation_error_rgba8_dev); the element count is 3 * f*(H//f) * f*(W//f)."""
        import torch
        assert hr.is_cuda and hr.dtype == torch.uint8 and hr.is_contiguous() and hr.dim() == 3
        h, w, c = hr.shape
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=hr.device)
        _lib.check(self._L.sr_validation_error_rgba8_dev(self._ctx, C.c_void_p(hr.data_ptr()), c, h, w, int(bool(linear_loss)),
                                                         C.c_void_p(out.data_ptr()), self._stream_ptr(stream, hr.device)), self._ctx)
        return out

    # ---- pairs: the LR image is the caller's, not the pool of the HR image (include/srhip.h, "Pairs") ----
    def _pair_shapes(self, lr_shape, hr_shape):
        """(lh, lw) of a pair or a batch of pairs whose trailing dimensions are (h, w, c); the HR size must be exactly f x the LR size."""
        f = self.factor
        lh, lw = lr_shape[-3], lr_shape[-2]
        if tuple(lr_shape[:-3]) != tuple(hr_shape[:-3]) or (hr_shape[-3], hr_shape[-2]) != (f * lh, f * lw):
            raise _lib.SrError(_lib.SR_E_INVALID, f"HR {tuple(hr_shape)} is not {f} x LR {tuple(lr_shape)}")
        return lh, lw

    def validation_error_pair(self, lr: np.ndarray, hr: np.ndarray, linear_loss: bool = False, members=None):
        """LR image (lh,lw,3|4) and HR image (f*lh,f*lw,3|4), both u8 (byte / 255, alpha dropped) or both (.,.,3) f32 ->
        (err_sum, n_elems): the squared error of sr_net(f)(lr) against hr (sr_pair_validation_error_*).  members: None, or the mask of a
        self-ensemble whose output is scored in the network's place (u8 pairs only; sr_pair_validation_error_ensemble_rgba8)."""
        lr, hr = np.asarray(lr), np.asarray(hr)
        if lr.ndim != 3 or hr.ndim != 3:
            raise ValueError("expected one (H, W, C) image each")
        if lr.dtype != hr.dtype:
            raise ValueError("LR and HR must both be u8 or both f32")
        lh, lw = self._pair_shapes(lr.shape, hr.shape)
        err, n = C.c_double(), C.c_size_t()
        lr, hr = np.ascontiguousarray(lr), np.ascontiguousarray(hr)
        if members is not None:
            if hr.dtype != np.uint8:
                raise ValueError("the ensemble form takes u8 pixels")
            u8p = C.POINTER(C.c_uint8)
            st = self._L.sr_pair_validation_error_ensemble_rgba8(self._ctx, lr.ctypes.data_as(u8p), lr.shape[2], hr.ctypes.data_as(u8p),
                                                                 hr.shape[2], lh, lw, int(bool(linear_loss)), self._members(members),
                                                                 C.byref(err), C.byref(n))
        elif hr.dtype == np.uint8:
            u8p = C.POINTER(C.c_uint8)
            st = self._L.sr_pair_validation_error_rgba8(self._ctx, lr.ctypes.data_as(u8p), lr.shape[2], hr.ctypes.data_as(u8p), hr.shape[2],
                                                        lh, lw, int(bool(linear_loss)), C.byref(err), C.byref(n))
        elif hr.dtype == np.float32:
            if lr.shape[2] != 3 or hr.shape[2] != 3:
                raise ValueError("an f32 image has 3 channels")
            fp = C.POINTER(C.c_float)
            st = self._L.sr_pair_validation_error_f32(self._ctx, lr.ctypes.data_as(fp), hr.ctypes.data_as(fp), lh, lw, int(bool(linear_loss)),
                                                      C.byref(err), C.byref(n))
        else:
            raise ValueError("expected u8 or f32 pixels")
        _lib.check(st, self._ctx)
        return err.value, n.value

    def validation_error_pair_dev(self, lr, hr, linear_loss: bool = False, out=None, stream=None):
        """(lh,lw,3|4) and (f*lh,f*lw,3|4) u8 torch tensors on this engine's device -> a float64 tensor of one element holding err_sum,
        asynchronous on the stream (sr_pair_validation_error_rgba8_dev)."""
        import torch
        for t in (lr, hr):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3
        lh, lw = self._pair_shapes(lr.shape, hr.shape)
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=hr.device)
        _lib.check(self._L.sr_pair_validation_error_rgba8_dev(self._ctx, C.c_void_p(lr.data_ptr()), lr.shape[2], C.c_void_p(hr.data_ptr()),
                                                              hr.shape[2], lh, lw, int(bool(linear_loss)), C.c_void_p(out.data_ptr()),
                                                              self._stream_ptr(stream, hr.device)), self._ctx)
        return out

    def backprop_pair(self, lr: np.ndarray, hr: np.ndarray, params, linear_loss: bool = False, loss_scale: Optional[float] = None,
                      l2: float = 0.0):
        """LR batch (n,lh,lw,3|4) and HR batch (n,f*lh,f*lw,3|4), both u8 or both (.,.,.,3) f32 -> (err_sum, n_elems, grad), as
        backprop() with the network's input taken from lr (sr_pair_backprop_*).  loss_scale None: 1 / n_elems."""
        lr, hr = np.asarray(lr), np.asarray(hr)
        if lr.ndim == 3 and hr.ndim == 3:
            lr, hr = lr[None], hr[None]
        if lr.ndim != 4 or hr.ndim != 4:
            raise ValueError("expected (n, H, W, C) images")
        if lr.dtype != hr.dtype:
            raise ValueError("LR and HR must both be u8 or both f32")
        lh, lw = self._pair_shapes(lr.shape, hr.shape)
        n, f = hr.shape[0], self.factor
        if loss_scale is None:
            loss_scale = 1.0 / (n * 3 * f * lh * f * lw) if lh >= 1 and lw >= 1 and n >= 1 else 1.0
        p = np.ascontiguousarray(params, dtype=np.float32)
        grad = np.empty(max(self.num_params(), 1), dtype=np.float32)
        err, ne = C.c_double(), C.c_size_t()
        fp = C.POINTER(C.c_float)
        lr, hr = np.ascontiguousarray(lr), np.ascontiguousarray(hr)
        if hr.dtype == np.uint8:
            u8p = C.POINTER(C.c_uint8)
            st = self._L.sr_pair_backprop_rgba8(self._ctx, p.ctypes.data_as(fp), p.size, lr.ctypes.data_as(u8p), lr.shape[3],
                                                hr.ctypes.data_as(u8p), hr.shape[3], n, lh, lw, int(bool(linear_loss)), float(loss_scale),
                                                float(l2), C.byref(err), C.byref(ne), grad.ctypes.data_as(fp))
        elif hr.dtype == np.float32:
            if lr.shape[3] != 3 or hr.shape[3] != 3:
                raise ValueError("an f32 batch has 3 channels")
            st = self._L.sr_pair_backprop_f32(self._ctx, p.ctypes.data_as(fp), p.size, lr.ctypes.data_as(fp), hr.ctypes.data_as(fp), n, lh, lw,
                                              int(bool(linear_loss)), float(loss_scale), float(l2), C.byref(err), C.byref(ne),
                                              grad.ctypes.data_as(fp))
        else:
            raise ValueError("expected u8 or f32 pixels")
        _lib.check(st, self._ctx)
        return err.value, ne.value, grad

    def backprop_pair_dev(self, lr, hr, params, linear_loss: bool = False, loss_scale: Optional[float] = None, l2: float = 0.0,
                          grad=None, err=None, stream=None):
        """(n,lh,lw,3|4) and (n,f*lh,f*lw,3|4) u8 torch tensors and an f32 parameter tensor on this engine's device -> (err, grad),
        asynchronous on the stream (sr_pair_backprop_rgba8_dev)."""
        import torch
        for t in (lr, hr):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 4
        assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()
        lh, lw = self._pair_shapes(lr.shape, hr.shape)
        n, f = hr.shape[0], self.factor
        if loss_scale is None:
            loss_scale = 1.0 / (n * 3 * f * lh * f * lw) if lh >= 1 and lw >= 1 and n >= 1 else 1.0
        if grad is None:
            grad = torch.empty_like(params)
        if err is None:
            err = torch.empty(1, dtype=torch.float64, device=hr.device)
        if params.numel() != self.num_params():
            raise _lib.SrError(_lib.SR_E_PARAM_COUNT)
        _lib.check(self._L.sr_pair_backprop_rgba8_dev(self._ctx, C.c_void_p(params.data_ptr()), C.c_void_p(lr.data_ptr()), lr.shape[3],
                                                      C.c_void_p(hr.data_ptr()), hr.shape[3], n, lh, lw, int(bool(linear_loss)),
                                                      float(loss_scale), float(l2), C.c_void_p(err.data_ptr()),
                                                      C.c_void_p(grad.data_ptr()), self._stream_ptr(stream, hr.device)), self._ctx)
        return err, grad

    # ---- metrics: Y-channel PSNR and SSIM of the benchmark protocol (include/srhip.h, "Metrics") ----
    @staticmethod
    def _metrics_dict(m):
        return {"y_sq_err": int(m.y_sq_err), "y_count": int(m.y_count), "ssim_sum": float(m.ssim_sum), "ssim_count": int(m.ssim_count),
                "y_psnr": y_psnr(int(m.y_sq_err), int(m.y_count)), "ssim": ssim_mean(float(m.ssim_sum), int(m.ssim_count))}

    def image_metrics(self, a: np.ndarray, b: np.ndarray, shave=None):
        """Two (H,W,3|4) u8 images, a the scored one and b the ground truth -> a dict of y_sq_err, y_count, ssim_sum, ssim_count and the
        image's y_psnr and ssim (None where the count is 0).  shave None: the engine's factor.  No network runs (sr_image_metrics_rgba8)."""
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.ndim != 3 or b.ndim != 3 or a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape[:2] != b.shape[:2]:
            raise ValueError("expected two (H, W, C) u8 images of one size")
        m = _lib.Metrics()
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_image_metrics_rgba8(self._ctx, a.ctypes.data_as(u8p), a.shape[2], b.ctypes.data_as(u8p), b.shape[2], a.shape[0],
                                                  a.shape[1], -1 if shave is None else int(shave), C.byref(m)), self._ctx)
        return self._metrics_dict(m)

    def image_metrics_dev(self, a, b, shave=None, out=None, stream=None):
        """Two (H,W,3|4) u8 torch tensors on this engine's device -> a uint8 tensor of 16 bytes, the uint64 y_sq_err then the float64
        ssim_sum (metrics_from_bytes reads them), asynchronous on the stream (sr_image_metrics_rgba8_dev).  out: 16 bytes at a 4-byte
        aligned address."""
        import torch
        for t in (a, b):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3
        assert a.shape[:2] == b.shape[:2]
        if out is None:
            out = torch.empty(16, dtype=torch.uint8, device=a.device)
        _lib.check(self._L.sr_image_metrics_rgba8_dev(self._ctx, C.c_void_p(a.data_ptr()), a.shape[2], C.c_void_p(b.data_ptr()), b.shape[2],
                                                      a.shape[0], a.shape[1], -1 if shave is None else int(shave),
                                                      C.c_void_p(out.data_ptr()), self._stream_ptr(stream, a.device)), self._ctx)
        return out

    def validation_metrics(self, hr: np.ndarray, lr=None, linear_loss: bool = False, members=None, shave=None):
        """validation_error (lr None) or validation_error_pair of u8 images, and the scores of the same run of the network: the
        quantised output against the HR crop.  -> a dict of err_sum, n_elems (the bits of those calls), y_sq_err, y_count, ssim_sum,
        ssim_count, y_psnr, ssim.  shave None: the factor.  (sr_pool_validation_metrics_rgba8 / sr_pair_validation_metrics_rgba8)"""
        hr = np.ascontiguousarray(hr)
        if hr.ndim != 3 or hr.dtype != np.uint8:
            raise ValueError("expected one (H, W, C) u8 image")
        err, n, m = C.c_double(), C.c_size_t(), _lib.Metrics()
        u8p = C.POINTER(C.c_uint8)
        mask = 0 if members is None else self._members(members)
        s = -1 if shave is None else int(shave)
        if lr is None:
            st = self._L.sr_pool_validation_metrics_rgba8(self._ctx, hr.ctypes.data_as(u8p), hr.shape[2], hr.shape[0], hr.shape[1],
                                                     int(bool(linear_loss)), mask, s, C.byref(err), C.byref(n), C.byref(m))
        else:
            lr = np.ascontiguousarray(lr)
            if lr.ndim != 3 or lr.dtype != np.uint8:
                raise ValueError("expected one (H, W, C) u8 image")
            lh, lw = self._pair_shapes(lr.shape, hr.shape)
            st = self._L.sr_pair_validation_metrics_rgba8(self._ctx, lr.ctypes.data_as(u8p), lr.shape[2], hr.ctypes.data_as(u8p), hr.shape[2],
                                                          lh, lw, int(bool(linear_loss)), mask, s, C.byref(err), C.byref(n), C.byref(m))
        _lib.check(st, self._ctx)
        out = {"err_sum": err.value, "n_elems": n.value}
        out.update(self._metrics_dict(m))
        return out

    def validation_metrics_dev(self, hr, lr=None, linear_loss: bool = False, shave=None, err=None, out=None, stream=None):
        """The device form: (H,W,3|4) u8 torch tensors -> (a float64 tensor of one element holding err_sum, a uint8 tensor of the 16
        result bytes), asynchronous on the stream (sr_pool_validation_metrics_rgba8_dev / sr_pair_validation_metrics_rgba8_dev)."""
        import torch
        for t in (hr,) if lr is None else (hr, lr):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3
        if err is None:
            err = torch.empty(1, dtype=torch.float64, device=hr.device)
        if out is None:
            out = torch.empty(16, dtype=torch.uint8, device=hr.device)
        s = -1 if shave is None else int(shave)
        if lr is None:
            st = self._L.sr_pool_validation_metrics_rgba8_dev(self._ctx, C.c_void_p(hr.data_ptr()), hr.shape[2], hr.shape[0], hr.shape[1],
                                                         int(bool(linear_loss)), s, C.c_void_p(err.data_ptr()), C.c_void_p(out.data_ptr()),
                                                         self._stream_ptr(stream, hr.device))
        else:
            lh, lw = self._pair_shapes(lr.shape, hr.shape)
            st = self._L.sr_pair_validation_metrics_rgba8_dev(self._ctx, C.c_void_p(lr.data_ptr()), lr.shape[2], C.c_void_p(hr.data_ptr()),
                                                              hr.shape[2], lh, lw, int(bool(linear_loss)), s, C.c_void_p(err.data_ptr()),
                                                              C.c_void_p(out.data_ptr()), self._stream_ptr(stream, hr.device))
        _lib.check(st, self._ctx)
        return err, out

    def validation_nodes(self, h: int, w: int):
        """The last validation call's `input` node (the pooled LR image, (h//f, w//f, 3)) and `output` node (the f32 network output,
        (f*(h//f), f*(w//f), 3)), for an HR image of h x w (sr_read_validation_nodes)."""
        f = self.factor
        lr = np.empty((h // f, w // f, 3), dtype=np.float32)
        out = np.empty((f * (h // f), f * (w // f), 3), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._L.sr_read_validation_nodes(self._ctx, lr.ctypes.data_as(fp), lr.size, out.ctypes.data_as(fp), out.size), self._ctx)
        return lr, out

    # ---- training: backpropagation of the training graph (reference main.rs:181-257, network.rs:78-103) and one Adam step ----
    def num_params(self) -> int:
        return self._L.sr_num_params_factor(self.factor)

    def set_params(self, params):
        """Replace the inference weights (sr_set_params; synchronous -- finish this engine's own *_dev work first)."""
        p = np.ascontiguousarray(params, dtype=np.float32)
        _lib.check(self._L.sr_set_params(self._ctx, p.ctypes.data_as(C.POINTER(C.c_float)), p.size), self._ctx)

    def backprop(self, hr: np.ndarray, params, linear_loss: bool = False, loss_scale: Optional[float] = None, l2: float = 0.0):
        """HR batch (n,H,W,3|4) u8 (byte / 255, alpha dropped) or (n,H,W,3) f32 -> (err_sum, n_elems, grad): the squared error of
        sr_net(f) on the pooled batch against its f*(H//f) x f*(W//f) crop (of SrgbToLinear of both with linear_loss) and the gradient
        of loss_scale * err_sum + l2 * sum(p^2) at `params` (sr_backprop_*).  loss_scale None: 1 / n_elems (MseLoss's mean; UNPINNED)."""
        hr = np.asarray(hr)
        if hr.ndim == 3:
            hr = hr[None]
        if hr.ndim != 4:
            raise ValueError("expected (n, H, W, C) images")
        n, h, w, c = hr.shape
        f = self.factor
        if loss_scale is None:
            loss_scale = 1.0 / (n * 3 * (f * (h // f)) * (f * (w // f))) if h >= f and w >= f else 1.0
        p = np.ascontiguousarray(params, dtype=np.float32)
        grad = np.empty(max(self.num_params(), 1), dtype=np.float32)
        err, ne = C.c_double(), C.c_size_t()
        fp = C.POINTER(C.c_float)
        if hr.dtype == np.uint8:
            hr = np.ascontiguousarray(hr)
            st = self._L.sr_backprop_rgba8(self._ctx, p.ctypes.data_as(fp), p.size, hr.ctypes.data_as(C.POINTER(C.c_uint8)), c, n, h, w,
                                           int(bool(linear_loss)), float(loss_scale), float(l2), C.byref(err), C.byref(ne),
                                           grad.ctypes.data_as(fp))
        elif hr.dtype == np.float32:
            if c != 3:
                raise ValueError("an f32 HR batch has 3 channels")
            hr = np.ascontiguousarray(hr)
            st = self._L.sr_backprop_f32(self._ctx, p.ctypes.data_as(fp), p.size, hr.ctypes.data_as(fp), n, h, w, int(bool(linear_loss)),
                                         float(loss_scale), float(l2), C.byref(err), C.byref(ne), grad.ctypes.data_as(fp))
        else:
            raise ValueError("expected u8 or f32 pixels")
        _lib.check(st, self._ctx)
        return err.value, ne.value, grad

    def backprop_dev(self, hr, params, linear_loss: bool = False, loss_scale: Optional[float] = None, l2: float = 0.0,
                     grad=None, err=None, stream=None):
        """(n,H,W,3|4) u8 torch tensor and an f32 parameter tensor on this engine's device -> (err, grad): a float64 tensor of one
        element (err_sum) and the f32 gradient, asynchronous on the stream (sr_backprop_rgba8_dev)."""
        import torch
        assert hr.is_cuda and hr.dtype == torch.uint8 and hr.is_contiguous() and hr.dim() == 4
        assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous() and params.numel() == self.num_params()
        n, h, w, c = hr.shape
        f = self.factor
        if loss_scale is None:
            loss_scale = 1.0 / (n * 3 * (f * (h // f)) * (f * (w // f))) if h >= f and w >= f else 1.0
        if grad is None:
            grad = torch.empty_like(params)
        if err is None:
            err = torch.empty(1, dtype=torch.float64, device=hr.device)
        _lib.check(self._L.sr_backprop_rgba8_dev(self._ctx, C.c_void_p(params.data_ptr()), C.c_void_p(hr.data_ptr()), c, n, h, w,
                                                 int(bool(linear_loss)), float(loss_scale), float(l2), C.c_void_p(err.data_ptr()),
                                                 C.c_void_p(grad.data_ptr()), self._stream_ptr(stream, hr.device)), self._ctx)
        return err, grad

    def adam_step_dev(self, params, m, v, grad, step: int, lr: float = 2e-3, beta1: float = 0.95, beta2: float = 0.995,
                      eps: float = 1e-7, stream=None):
        """One Adam step in place on f32 torch tensors of one size (sr_adam_step_dev; defaults: the reference's, main.rs:199-205)."""
        import torch
        for t in (params, m, v, grad):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == params.numel()
        vp = C.c_void_p
        _lib.check(self._L.sr_adam_step_dev(self._ctx, vp(params.data_ptr()), vp(m.data_ptr()), vp(v.data_ptr()), vp(grad.data_ptr()),
                                            params.numel(), int(step), float(lr), float(beta1), float(beta2), float(eps),
                                            self._stream_ptr(stream, params.device)), self._ctx)

    def grad_norm_dev(self, grad, clip: float = 0.0, out=None, stream=None):
        """The f64 sum of squares of an f32 torch tensor on this engine's device, the clipping scale for `clip` (0: none) and the skip
        flag, as a 16-byte uint8 tensor holding one sr_grad_norm (sr_grad_norm_dev; asynchronous on the stream).  read_grad_norm(out)
        waits and decodes it."""
        import torch
        assert grad.is_cuda and grad.dtype == torch.float32 and grad.is_contiguous()
        if out is None:
            out = torch.empty(16, dtype=torch.uint8, device=grad.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.numel() >= 16
        vp = C.c_void_p
        _lib.check(self._L.sr_grad_norm_dev(self._ctx, vp(grad.data_ptr()), grad.numel(), float(clip), vp(out.data_ptr()),
                                            self._stream_ptr(stream, grad.device)), self._ctx)
        return out

    @staticmethod
    def read_grad_norm(out) -> dict:
        """{"sumsq", "scale", "skip"} of grad_norm_dev's result (waits for it)."""
        g = _lib.GradNorm.from_buffer_copy(out.cpu().numpy().tobytes()[:16])
        return {"sumsq": g.sumsq, "scale": float(np.float32(g.scale)), "skip": int(g.skip)}

    def adam_step_clipped_dev(self, params, m, v, grad, step: int, lr: float = 2e-3, beta1: float = 0.95, beta2: float = 0.995,
                              eps: float = 1e-7, norm=None, ema=None, ema_decay: float = 0.0, skipped=None, stream=None):
        """adam_step_dev on scale * grad, scale and skip read on the device from `norm` (grad_norm_dev's result; None: scale 1), then
        ema <- ema_decay ema + (1 - ema_decay) params where `ema` is given; a skipped step writes nothing and adds 1 to `skipped`, a
        one-element int64 tensor (sr_adam_step_clipped_dev)."""
        import torch
        for t in (params, m, v, grad) + ((ema,) if ema is not None else ()):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == params.numel()
        if skipped is not None:
            assert skipped.is_cuda and skipped.dtype == torch.int64 and skipped.numel() >= 1
        vp = C.c_void_p
        ptr = lambda t: vp(t.data_ptr()) if t is not None else None
        _lib.check(self._L.sr_adam_step_clipped_dev(self._ctx, vp(params.data_ptr()), vp(m.data_ptr()), vp(v.data_ptr()), vp(grad.data_ptr()),
                                                    params.numel(), int(step), float(lr), float(beta1), float(beta2), float(eps), ptr(norm),
                                                    ptr(ema), float(ema_decay), ptr(skipped), self._stream_ptr(stream, params.device)),
                   self._ctx)

    # ---- introspection ------------------------------------------------------
    def read_feature(self, which: int, h: int, w: int) -> np.ndarray:
        """Post-activation node data of the last call: 0..3 = f, l1, l2, l3."""
        out = np.empty((h, w, 32), dtype=np.float32)
        _lib.check(self._L.sr_read_feature(self._ctx, which, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), self._ctx)
        return out

    def set_pipeline(self, on: bool):
        """Host-pointer entry points: chunked upload / compute / download overlap (default on);
        results do not depend on it."""
        _lib.check(self._L.sr_set_pipeline(self._ctx, 1 if on else 0))

    def set_experiment(self, key: str, value: str = ""):
        """sr_set_experiment: "th" / "pipe" / "bw" A/B switches, "auxgrid", "cus" (results do not depend on them)."""
        _lib.check(self._L.sr_set_experiment(self._ctx, key.encode(), value.encode()))

    def get_experiment(self, key: str) -> str:
        """sr_get_experiment: what a switch has learned ("forktune": one line per shape the fork tuner has met; "plan": what the
        last call ran).  A buffer that is too small is refused like an unknown key: retried with larger ones up to 16 MB."""
        cap = 4096
        while True:
            buf = C.create_string_buffer(cap)
            st = self._L.sr_get_experiment(self._ctx, key.encode(), buf, len(buf))
            if st != _lib.SR_E_INVALID or cap >= 1 << 24:
                break
            cap *= 4
        _lib.check(st)
        return buf.value.decode()

    def last_plan(self) -> dict:
        """What the last call on this context ran (sr_get_experiment "plan"), as data: parse_plan of its text."""
        return parse_plan(self.get_experiment("plan"))

    def set_profiling(self, on: bool):
        _lib.check(self._L.sr_set_profiling(self._ctx, int(on)))

    def last_timing(self):
        tot, h2d, d2h = C.c_double(), C.c_double(), C.c_double()
        st = (C.c_double * 5)()
        _lib.check(self._L.sr_last_timing(self._ctx, C.byref(tot), st, C.byref(h2d), C.byref(d2h)))
        return {"total_ms": tot.value, "stage_ms": list(st), "h2d_ms": h2d.value, "d2h_ms": d2h.value}

    def device_info(self):
        name = C.create_string_buffer(128)
        cus, mhz = C.c_int(), C.c_int()
        _lib.check(self._L.sr_device_info(self._ctx, name, 128, C.byref(cus), C.byref(mhz)))
        return {"name": name.value.decode(), "compute_units": cus.value, "clock_mhz": mhz.value}


def upscale_multi(engines, px: np.ndarray, out: np.ndarray = None) -> np.ndarray:
    """One image over several engines (normally one per GPU) from this process: sr_upscale_*_multi.  px (H,W,3|4) u8
    -> (3H,3W,4) u8 RGBA, or (H,W,3) f32 -> (3H,3W,3) f32; bit-identical to the single-engine call."""
    L = _lib.lib()
    arr = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
    f = engines[0].factor
    if px.dtype == np.uint8:
        px = np.ascontiguousarray(px)
        h, w, c = px.shape
        if out is None:
            out = np.empty((f * h, f * w, 4), dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(L.sr_upscale_rgba8_multi(arr, len(engines), px.ctypes.data_as(u8p), c, h, w, out.ctypes.data_as(u8p)))
    else:
        px = np.ascontiguousarray(px, dtype=np.float32)
        h, w, c = px.shape
        if c != 3:
            raise ValueError("expected 3 channels")
        if out is None:
            out = np.empty((f * h, f * w, 3), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(L.sr_upscale_f32_multi(arr, len(engines), px.ctypes.data_as(fp), h, w, out.ctypes.data_as(fp)))
    return out


def upscale_batch_multi(engines, px: np.ndarray, out: np.ndarray = None) -> np.ndarray:
    """A batch dealt over several engines from this process (sr_upscale_*_batch_multi): image i -> engines[i mod N].
    px (n,H,W,3|4) u8 -> (n,3H,3W,4) u8 RGBA, or (n,H,W,3) f32 -> (n,3H,3W,3) f32; identical to one engine's result."""
    L = _lib.lib()
    arr = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
    f = engines[0].factor
    if px.dtype == np.uint8:
        px = np.ascontiguousarray(px)
        n, h, w, c = px.shape
        if out is None:
            out = np.empty((n, f * h, f * w, 4), dtype=np.uint8)
        u8p = C.POINTER(C.c_uint8)
        _lib.check(L.sr_upscale_rgba8_batch_multi(arr, len(engines), px.ctypes.data_as(u8p), c, n, h, w, out.ctypes.data_as(u8p)))
    else:
        px = np.ascontiguousarray(px, dtype=np.float32)
        n, h, w, c = px.shape
        if c != 3:
            raise ValueError("expected 3 channels")
        if out is None:
            out = np.empty((n, f * h, f * w, 3), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(L.sr_upscale_f32_batch_multi(arr, len(engines), px.ctypes.data_as(fp), n, h, w, out.ctypes.data_as(fp)))
    return out


def comm_init_all(engines, transport: str = "rccl"):
    """One process, several engines; engine k becomes rank k.  transport "rccl": ncclCommInitAll inside libsrhip, one
    engine per device.  "local": sr_comm_init_local -- halos by peer copy on each engine's own stream, no RCCL, and the
    same device may carry several engines."""
    if transport not in ("rccl", "local"):
        raise ValueError("transport must be 'rccl' or 'local'")
    arr = (C.c_void_p * len(engines))(*[e._ctx for e in engines])
    fn = _lib.lib().sr_comm_init_all if transport == "rccl" else _lib.lib().sr_comm_init_local
    _lib.check(fn(arr, len(engines)), engines[0]._ctx)


def upscale_sharded_all(engines, bands, outs=None):
    """Bands (torch tensors, band k on engine k's device, rank order) of ONE image -> their output rows, through
    sr_upscale_sharded_*_all (halo exchange over the transport comm_init_all chose + band passes, synchronous)."""
    import torch
    n = len(engines)
    f = engines[0].factor
    u8 = bands[0].dtype == torch.uint8
    w, c = bands[0].shape[1], bands[0].shape[2]
    if outs is None:
        outs = [torch.empty((f * b.shape[0], f * w, 4 if u8 else 3), dtype=b.dtype, device=b.device) for b in bands]
    ctxs = (C.c_void_p * n)(*[e._ctx for e in engines])
    bp = (C.c_void_p * n)(*[b.data_ptr() for b in bands])
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    hb = (C.c_int * n)(*[b.shape[0] for b in bands])
    L = _lib.lib()
    for b in bands:
        torch.cuda.synchronize(b.device)  # the library runs on the contexts' own streams
    if u8:
        _lib.check(L.sr_upscale_sharded_rgba8_all(ctxs, n, bp, c, hb, w, op), engines[0]._ctx)
    else:
        _lib.check(L.sr_upscale_sharded_f32_all(ctxs, n, bp, hb, w, op), engines[0]._ctx)
    return outs


DEGRADE_KEYS = {"blur": (0.0, float(_lib.SR_DEGRADE_MAX_SIGMA), False), "noise": (0.0, float(_lib.SR_DEGRADE_MAX_NOISE), False),
                "jpeg": (0, 100, True)}
_GOLDEN, _MASK64 = 0x9E3779B97F4A7C15, 2 ** 64 - 1


def parse_degrade_spec(text: str) -> dict:
    """'blur=A[:B],noise=A[:B],jpeg=A[:B]' (the CLI's --degrade) -> {"blur": (A, B), "noise": (A, B), "jpeg": (A, B)}; a key that is
    absent is (0, 0): that stage is off.  A malformed spec, a reversed or an out-of-range range is a ValueError that names the key."""
    import math
    import re
    out = {k: ((0, 0) if integer else (0.0, 0.0)) for k, (_, _, integer) in DEGRADE_KEYS.items()}
    seen = set()
    if not text:
        raise ValueError("--degrade: empty spec")
    for part in text.split(","):
        key, eq, val = part.partition("=")
        if key not in DEGRADE_KEYS:
            raise ValueError(f"--degrade: unknown key '{key}'")
        if not eq or key in seen:
            raise ValueError(f"--degrade: malformed or repeated key '{key}'")
        seen.add(key)
        lo, hi, integer = DEGRADE_KEYS[key]
        try:
            if not all(re.fullmatch(r"[+-]?\d+" if integer else r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", v) for v in val.split(":")):
                raise ValueError(val)
            ab = [int(v) if integer else float(v) for v in val.split(":")]
        except ValueError:
            raise ValueError(f"--degrade: malformed value for '{key}'") from None
        if len(ab) not in (1, 2) or any(not math.isfinite(v) for v in ab):
            raise ValueError(f"--degrade: malformed value for '{key}'")
        a, b = ab[0], ab[-1]
        if b < a:
            raise ValueError(f"--degrade: reversed range for '{key}'")
        if a < lo or b > hi:
            raise ValueError(f"--degrade: range for '{key}' outside {lo}..{hi}")
        out[key] = (a, b)
    return out


LOSS_EPS_DEFAULT = 1e-3


def _check_loss_eps(eps) -> float:
    """Charbonnier's eps as the f32 the library takes: finite, 0 < eps <= 1 (ValueError otherwise)."""
    try:
        e = float(np.float32(eps))
    except (TypeError, ValueError):
        raise ValueError(f"loss: eps must be a number, got {eps!r}") from None
    if not (0.0 < e <= 1.0):   # (a NaN fails both comparisons)
        raise ValueError(f"loss: eps must be finite with 0 < eps <= 1, got {eps!r}")
    return e


def parse_loss_spec(text: str):
    """'mse' | 'l1' | 'charbonnier[:EPS]' (the CLI's --loss) -> (kind, eps), the arguments of Engine.set_loss; eps is 1e-3 where the
    spec has none.  Anything else -- an unknown kind, an EPS on a kind that has none, an EPS that is not a plain decimal in (0, 1] -- is a
    ValueError that names --loss."""
    import re
    kind, colon, val = text.partition(":")
    if kind not in Engine.LOSSES:
        raise ValueError(f"--loss: unknown kind '{kind}' (mse, l1, charbonnier[:EPS])")
    if not colon:
        return kind, LOSS_EPS_DEFAULT
    if kind != "charbonnier":
        raise ValueError(f"--loss: '{kind}' takes no EPS")
    if not re.fullmatch(r"\+?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", val):
        raise ValueError(f"--loss: malformed EPS '{val}'")
    try:
        return kind, _check_loss_eps(float(val))
    except (ValueError, OverflowError):
        raise ValueError(f"--loss: EPS '{val}' outside 0 < EPS <= 1") from None


_LR_NUM = r"\+?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?"


def parse_lr_schedule(text: str, base: float = 2e-3, warmup: int = 0):
    """'constant' | 'step:EVERY:GAMMA' | 'cosine:TOTAL[:MIN]' (the CLI's --lr-schedule) with the base rate (--lr) and the warm-up steps
    (--warmup) -> the sr_lr_schedule that lr_at takes.  EVERY and TOTAL are whole numbers >= 1, 0 < GAMMA <= 1, 0 <= MIN <= base.  Anything
    else is a ValueError that names the option."""
    import math
    import re
    try:
        b = float(np.float32(base))
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"--lr: expected a number, got {base!r}") from None
    if not math.isfinite(b) or b < 0:
        raise ValueError(f"--lr: must be finite and at least 0, got {base!r}")
    if isinstance(warmup, bool) or not isinstance(warmup, (int, np.integer)) or warmup < 0 or warmup >= 2 ** 62:
        raise ValueError(f"--warmup: expected a whole number of steps >= 0, got {warmup!r}")
    s = _lib.LrSchedule(_lib.SR_LR_CONSTANT, b, int(warmup), 0, 0.0, 0, 0.0)
    parts = str(text).split(":")
    whole = lambda v: re.fullmatch(r"\+?\d{1,18}", v) and int(v) >= 1
    if parts == ["constant"]:
        return s
    if parts[0] == "step" and len(parts) == 3:
        if not whole(parts[1]):
            raise ValueError(f"--lr-schedule: EVERY must be a whole number >= 1, got '{parts[1]}'")
        if not re.fullmatch(_LR_NUM, parts[2]) or not (0.0 < float(parts[2]) <= 1.0):
            raise ValueError(f"--lr-schedule: GAMMA must be a number with 0 < GAMMA <= 1, got '{parts[2]}'")
        s.kind, s.every, s.gamma = _lib.SR_LR_STEP, int(parts[1]), float(parts[2])
        return s
    if parts[0] == "cosine" and len(parts) in (2, 3):
        if not whole(parts[1]):
            raise ValueError(f"--lr-schedule: TOTAL must be a whole number >= 1, got '{parts[1]}'")
        mn = 0.0
        if len(parts) == 3:
            if not re.fullmatch(_LR_NUM, parts[2]) or not (0.0 <= float(np.float32(float(parts[2]))) <= b):
                raise ValueError(f"--lr-schedule: MIN must be a number with 0 <= MIN <= the base rate, got '{parts[2]}'")
            mn = float(parts[2])
        s.kind, s.total, s.min_lr = _lib.SR_LR_COSINE, int(parts[1]), mn
        return s
    raise ValueError(f"--lr-schedule: expected constant, step:EVERY:GAMMA or cosine:TOTAL[:MIN], got '{text}'")


def lr_at(schedule, step: int) -> float:
    """The learning rate of step 1, 2, ... under a schedule of parse_lr_schedule, as the f32 the session takes (sr_lr_at: the one
    function the CLI uses too).  Host only."""
    out = C.c_float()
    _lib.check(_lib.lib().sr_lr_at(C.byref(schedule), int(step), C.byref(out)))
    return float(out.value)


def degrade_draws(spec, seed: int, count: int, first: int = 0):
    """Draws first .. first + count - 1 of a spec (a string or parse_degrade_spec's dict) under `seed`, as keyword arguments of
    Engine.degrade.  The stream is SplitMix64 seeded with seed ^ 0xD6E8FEB86659FD93, four outputs a draw -- blur, noise, jpeg, noise seed;
    value = A + u (B - A), jpeg = A + floor(u (B - A + 1)), u = (x >> 11) 2^-53; the fourth output is the noise seed as is."""
    import math
    if isinstance(spec, str):
        spec = parse_degrade_spec(spec)

    def output(j):
        z = ((seed ^ 0xD6E8FEB86659FD93) + j * _GOLDEN) & _MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        return z ^ (z >> 31)

    out = []
    for i in range(first, first + count):
        u = [(output(4 * i + j) >> 11) * 2.0 ** -53 for j in (1, 2, 3)]
        (a0, b0), (a1, b1), (a2, b2) = spec["blur"], spec["noise"], spec["jpeg"]
        out.append({"sigma": a0 + u[0] * (b0 - a0), "noise": a1 + u[1] * (b1 - a1), "quality": a2 + int(math.floor(u[2] * (b2 - a2 + 1))),
                    "seed": output(4 * i + 4)})
    return out


def validation_psnr(engines, images, linear_loss: bool = False, lr_images=None, members=None, degrade=None, seed: int = 0) -> float:
    """The reference's validation PSNR (main.rs:236-246) of a set of HR images: -10 log10(sum err_i / sum n_i).  Images are dealt
    round-robin over the engines (one host thread each); the sums are taken in image order, so the value does not depend on how many
    engines there are.  A zero error is +inf.  lr_images: the LR partner of each image -- the set is then scored as pairs
    (validation_error_pair) instead of by pooling.  members: None, or the mask of a self-ensemble that is scored in the network's place.
    degrade: a spec (the CLI's --degrade string, or parse_degrade_spec's dict) -- image i is cropped to a multiple of the factor, degraded
    whole on its engine with draw i of the spec under `seed` (degrade_draws) and scored as a pair with that LR image."""
    import math
    from concurrent.futures import ThreadPoolExecutor
    if isinstance(engines, Engine):
        engines = [engines]
    images = list(images)
    if not engines or not images:
        raise ValueError("validation_psnr needs at least one engine and one image")
    if lr_images is not None:
        lr_images = list(lr_images)
        if len(lr_images) != len(images):
            raise ValueError("validation_psnr needs one LR image per HR image")
    res = [None] * len(images)
    kw = {} if members is None else {"members": members}
    if degrade is not None:
        if lr_images is not None:
            raise ValueError("validation_psnr takes lr_images or degrade, not both")
        draws = degrade_draws(degrade, seed, len(images))

    def run(k):
        for i in range(k, len(images), len(engines)):
            if degrade is not None:
                f = engines[k].factor
                hr = np.ascontiguousarray(np.asarray(images[i])[:images[i].shape[0] // f * f, :images[i].shape[1] // f * f])
                res[i] = engines[k].validation_error_pair(engines[k].degrade(hr, f, **draws[i]), hr, linear_loss, **kw)
            elif lr_images is None:
                res[i] = engines[k].validation_error(images[i], linear_loss, **kw)
            else:
                res[i] = engines[k].validation_error_pair(lr_images[i], images[i], linear_loss, **kw)

    with ThreadPoolExecutor(max_workers=len(engines)) as pool:
        for fut in [pool.submit(run, k) for k in range(len(engines))]:
            fut.result()
    err = n = 0.0
    for e, m in res:
        err += e
        n += m
    return math.inf if err == 0.0 else -10.0 * math.log10(err / n)


def y_psnr(y_sq_err: int, y_count: int):
    """One image's Y-PSNR from its sums: 10 log10(255^2 y_count / y_sq_err); inf at zero error, None for an empty region."""
    import math
    if y_count == 0:
        return None
    return math.inf if y_sq_err == 0 else 10.0 * math.log10(65025.0 * y_count / y_sq_err)


def ssim_mean(ssim_sum: float, ssim_count: int):
    """One image's SSIM: ssim_sum / ssim_count; None where the region holds no window."""
    return None if ssim_count == 0 else ssim_sum / ssim_count


def metrics_from_bytes(result16, h: int, w: int, shave: int) -> dict:
    """The 16 bytes a *_dev metrics call wrote (uint64 y_sq_err, float64 ssim_sum) and the counts of an h x w image shaved by `shave`."""
    import struct
    y_sq_err, ssim_sum = struct.unpack("<Qd", bytes(bytearray(result16)))
    rh, rw = h - 2 * shave, w - 2 * shave
    y_count = rh * rw if rh > 0 and rw > 0 else 0
    ssim_count = (rh - 10) * (rw - 10) if rh >= 11 and rw >= 11 else 0
    return {"y_sq_err": y_sq_err, "y_count": y_count, "ssim_sum": ssim_sum, "ssim_count": ssim_count,
            "y_psnr": y_psnr(y_sq_err, y_count), "ssim": ssim_mean(ssim_sum, ssim_count)}


def aggregate_metrics(per_image) -> dict:
    """Per-image dicts (validation_metrics) in image order -> {"psnr": the pooled figure of validation_psnr, "y_psnr", "ssim": the means of
    the per-image values (a zero-error image contributes inf), "skipped": [(index, "y_psnr" | "ssim"), ...] for the images whose region
    was empty or held no window and which the mean leaves out}.  A mean over no image is None."""
    import math
    err = n = 0.0
    ys, ss, skipped = [], [], []
    for i, m in enumerate(per_image):
        err += m["err_sum"]
        n += m["n_elems"]
        if m["y_psnr"] is None:
            skipped.append((i, "y_psnr"))
        else:
            ys.append(m["y_psnr"])
        if m["ssim"] is None:
            skipped.append((i, "ssim"))
        else:
            ss.append(m["ssim"])
    return {"psnr": math.inf if err == 0.0 else -10.0 * math.log10(err / n),
            "y_psnr": math.fsum(ys) / len(ys) if ys else None,
            "ssim": math.fsum(ss) / len(ss) if ss else None, "skipped": skipped}


def validation_metrics(engines, images, lr_images=None, members=None, shave=None, linear_loss: bool = False) -> dict:
    """validation_psnr with the benchmark protocol's scores: images are dealt round-robin over the engines, each scored by
    Engine.validation_metrics, and the results aggregated in image order (aggregate_metrics), so the values do not depend on how many
    engines there are.  "per_image" holds the per-image dicts."""
    from concurrent.futures import ThreadPoolExecutor
    if isinstance(engines, Engine):
        engines = [engines]
    images = list(images)
    if not engines or not images:
        raise ValueError("validation_metrics needs at least one engine and one image")
    if lr_images is not None:
        lr_images = list(lr_images)
        if len(lr_images) != len(images):
            raise ValueError("validation_metrics needs one LR image per HR image")
    res = [None] * len(images)

    def run(k):
        for i in range(k, len(images), len(engines)):
            res[i] = engines[k].validation_metrics(images[i], None if lr_images is None else lr_images[i], linear_loss, members, shave)

    with ThreadPoolExecutor(max_workers=len(engines)) as pool:
        for fut in [pool.submit(run, k) for k in range(len(engines))]:
            fut.result()
    out = aggregate_metrics(res)
    out["per_image"] = res
    return out


def init_params(factor: int = FACTOR, seed: int = 0) -> np.ndarray:
    """The reference's g.init_params() for sr_net(factor) (sr_init_params; the seeded generator and the UNPINNED rules are in
    include/srhip.h).  Host only."""
    L = _lib.lib()
    n = L.sr_num_params_factor(factor)
    if n < 0:
        raise _lib.SrError(_lib.SR_E_FACTOR)
    out = np.empty(n, dtype=np.float32)
    _lib.check(L.sr_init_params(factor, seed & 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(C.POINTER(C.c_float)), n))
    return out


class Trainer:
    """Minibatch Adam on the GPU (the optimisation loop of the reference's `train`, main.rs:181-257) over a training session of the
    engine's context (sr_train_*): parameters, moments and an image store live on the engine's device.
    step(hr_batch) -> err_sum of that batch at the parameters before the step (synchronous); add_image / step_crops queue steps on
    random crops without waiting (sync() collects their err_sums).
    loss / loss_eps: the objective (Engine.set_loss), set on the ENGINE when the trainer is made -- it is state of the engine, not of
    the trainer: every backprop call and every trainer on that engine uses it until set_loss is called again.
    clip_norm / ema_decay (set_optim), set_lr, ema(), state() / load_state(), sync_stats(): gradient clipping, an average of the
    parameters, a rate per step and what a run needs to continue bit for bit (include/srhip.h "Optimiser"); all off by default, and
    the default trainer's steps are then launch for launch what they were."""

    def __init__(self, engine: Engine, start_params, linear_loss: bool = False, l2: float = 1e-6, lr: float = 2e-3,
                 beta1: float = 0.95, beta2: float = 0.995, eps: float = 1e-7, store_bytes: Optional[int] = None,
                 loss: str = "mse", loss_eps: float = LOSS_EPS_DEFAULT, clip_norm: float = 0.0, ema_decay: float = 0.0):
        p = np.ascontiguousarray(start_params, dtype=np.float32)
        if p.size != engine.num_params():
            raise ValueError(f"expected {engine.num_params()} parameters, got {p.size}")
        engine.set_loss(loss, loss_eps)
        self.engine = engine
        self._L = engine._L
        self._t = C.c_void_p()
        store = _lib.SR_TRAIN_STORE_AUTO if store_bytes is None else int(store_bytes)
        _lib.check(self._L.sr_train_create(C.byref(self._t), engine._ctx, p.ctypes.data_as(C.POINTER(C.c_float)), p.size,
                                           int(bool(linear_loss)), float(l2), float(lr), float(beta1), float(beta2), float(eps), store),
                   engine._ctx)
        self.linear_loss, self.l2, self.lr, self.beta1, self.beta2, self.eps = linear_loss, l2, lr, beta1, beta2, eps
        self.steps = 0
        self._pending = 0
        self.clip_norm, self.ema_decay = 0.0, 0.0
        if clip_norm or ema_decay:
            try:
                self.set_optim(clip_norm, ema_decay)
            except Exception:
                self.close()
                raise

    def set_optim(self, clip_norm: float = 0.0, ema_decay: float = 0.0) -> None:
        """Gradient clipping at an L2 norm of clip_norm (0: off) and an average of the parameters, e <- d e + (1 - d) p after every step
        (0: off; first enabled, e starts at the current parameters).  Waits for the steps in flight (sr_train_set_optim)."""
        _lib.check(self._L.sr_train_set_optim(self._t, float(clip_norm), float(ema_decay)), self.engine._ctx)
        self.clip_norm, self.ema_decay = float(clip_norm), float(ema_decay)

    def set_lr(self, lr: float) -> None:
        """The learning rate of the steps queued from now on; no waiting (sr_train_set_lr)."""
        _lib.check(self._L.sr_train_set_lr(self._t, float(lr)), self.engine._ctx)
        self.lr = float(lr)

    def ema(self) -> np.ndarray:
        """The averaged parameters (waits); an SrError while the average is off."""
        out = np.empty(self.engine.num_params(), dtype=np.float32)
        _lib.check(self._L.sr_train_ema(self._t, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), self.engine._ctx)
        return out

    def state(self) -> dict:
        """What a run needs besides params() to continue bit for bit (waits): {"m", "v", "e" (None while the average is off), "step",
        "skipped"} (sr_train_get_state)."""
        n = self.engine.num_params()
        fp = C.POINTER(C.c_float)
        m, v = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
        e = np.empty(n, dtype=np.float32) if self.ema_decay else None
        step, skipped = C.c_longlong(), C.c_longlong()
        _lib.check(self._L.sr_train_get_state(self._t, m.ctypes.data_as(fp), v.ctypes.data_as(fp), e.ctypes.data_as(fp) if e is not None else None,
                                              n, C.byref(step), C.byref(skipped)), self.engine._ctx)
        return {"m": m, "v": v, "e": e, "step": step.value, "skipped": skipped.value}

    def load_state(self, state: dict) -> None:
        """Continue from state() of a session with the same parameters and settings (sr_train_set_state); refused, the session stays as
        it was."""
        fp = C.POINTER(C.c_float)
        m, v = (np.ascontiguousarray(state[k], dtype=np.float32).ravel() for k in ("m", "v"))
        e = np.ascontiguousarray(state["e"], dtype=np.float32).ravel() if state.get("e") is not None else None
        if m.size != v.size or (e is not None and e.size != m.size):
            raise ValueError("m, v and e must have one size")
        _lib.check(self._L.sr_train_set_state(self._t, m.ctypes.data_as(fp), v.ctypes.data_as(fp), e.ctypes.data_as(fp) if e is not None else None,
                                              m.size, int(state["step"]), int(state.get("skipped", 0))), self.engine._ctx)
        self.steps = int(state["step"])

    def sync_stats(self) -> List[dict]:
        """sync() with {"err_sum", "grad_norm", "lr", "scale"} per step (grad_norm 0 while clipping is off); it shares sync()'s queue."""
        buf = (_lib.TrainStat * max(self._pending, 1))()
        n = C.c_size_t()
        _lib.check(self._L.sr_train_sync_stats(self._t, buf, len(buf), C.byref(n)), self.engine._ctx)
        self._pending = 0
        return [{"err_sum": b.err_sum, "grad_norm": b.grad_norm, "lr": float(b.lr), "scale": float(b.scale)} for b in buf[:min(n.value, len(buf))]]

    def add_image(self, px) -> int:
        """(h, w, 3|4) u8 -> the id of the image in the device store, or -1 when the store has no room."""
        px = np.ascontiguousarray(px)
        if px.dtype != np.uint8 or px.ndim != 3:
            raise ValueError("expected (h, w, 3|4) u8 pixels")
        h, w, c = px.shape
        i = C.c_int()
        _lib.check(self._L.sr_train_add_image(self._t, px.ctypes.data_as(C.POINTER(C.c_uint8)), c, h, w, C.byref(i)), self.engine._ctx)
        return i.value

    @staticmethod
    def _members(items):
        """The member of each item -- its optional fourth element, 0..7 -- as the u8 array the _aug entry points take, or None when no
        item has one (the plain call)."""
        if not any(len(it) > 3 for it in items):
            return None
        ks = [int(it[3]) if len(it) > 3 else 0 for it in items]
        if any(k < 0 or k > 7 for k in ks):
            raise ValueError("a member is one of the 8 flips and rotations, 0..7")
        return (C.c_uint8 * len(ks))(*ks)

    @staticmethod
    def _crop_items(items):
        """The sr_train_crop array of (image, y0, x0[, member]) items, and the pixel arrays it points into (to be kept alive for the call)."""
        arr = (_lib.TrainCrop * max(len(items), 1))()
        keep = []
        for k, (img, y0, x0) in enumerate(it[:3] for it in items):
            it = arr[k]
            it.y0, it.x0 = int(y0), int(x0)
            if isinstance(img, (int, np.integer)):
                it.image = int(img)
            else:
                px = np.ascontiguousarray(img)
                if px.dtype != np.uint8 or px.ndim != 3:
                    raise ValueError("expected (h, w, 3|4) u8 pixels")
                keep.append(px)
                it.image, it.px = -1, px.ctypes.data
                it.h, it.w, it.in_channels = px.shape
        return arr, keep

    def step_crops(self, items, crop_h: int, crop_w: int) -> None:
        """One step on crops, queued without waiting.  items: (image, y0, x0[, member]) with image an id of add_image or a (h, w, 3|4) u8
        array; member k (0..7, default 0) makes the item T_k of its window (sr_train_step_aug: the window of k >= 4 is crop_w x crop_h)."""
        members = self._members(items)
        arr, keep = self._crop_items(items)
        if members is None:
            rc = self._L.sr_train_step(self._t, arr, len(items), int(crop_h), int(crop_w))
        else:
            rc = self._L.sr_train_step_aug(self._t, arr, members, len(items), int(crop_h), int(crop_w))
        _lib.check(rc, self.engine._ctx)
        self.steps += 1
        self._pending += 1

    def step_degraded(self, items, degs, crop_h: int, crop_w: int) -> None:
        """One step on crops whose network input is degraded on the device, queued without waiting (sr_train_step_degrade).  items as in
        step_crops, (image, y0, x0[, member]); degs: one dict of sigma, noise, quality, seed (Engine.degrade's keywords, all optional) per
        item.  crop_h and crop_w are multiples of the engine's factor."""
        if len(degs) != len(items):
            raise ValueError("expected one degradation per item")
        members = self._members(items)
        arr, keep = self._crop_items(items)
        g = (_lib.Degrade * max(len(items), 1))()
        for k, d in enumerate(degs):
            g[k] = _lib.Degrade(float(d.get("sigma", 0.0)), float(d.get("noise", 0.0)), int(d.get("quality", 0)), int(d.get("seed", 0)) & (2 ** 64 - 1))
        _lib.check(self._L.sr_train_step_degrade(self._t, arr, members, g, len(items), int(crop_h), int(crop_w)), self.engine._ctx)
        self.steps += 1
        self._pending += 1

    def add_pair(self, lr, hr) -> int:
        """(lh, lw, 3|4) and (f*lh, f*lw, 3|4) u8 -> the id of the pair in the device store (one entry), or -1 when there is no room."""
        lr, hr = np.ascontiguousarray(lr), np.ascontiguousarray(hr)
        if lr.dtype != np.uint8 or hr.dtype != np.uint8 or lr.ndim != 3 or hr.ndim != 3:
            raise ValueError("expected (h, w, 3|4) u8 pixels")
        lh, lw = self.engine._pair_shapes(lr.shape, hr.shape)
        i = C.c_int()
        u8p = C.POINTER(C.c_uint8)
        _lib.check(self._L.sr_train_add_pair(self._t, lr.ctypes.data_as(u8p), lr.shape[2], hr.ctypes.data_as(u8p), hr.shape[2], lh, lw,
                                             C.byref(i)), self.engine._ctx)
        return i.value

    def step_pair_crops(self, items, crop_lh: int, crop_lw: int) -> None:
        """One step on crops of pairs, queued without waiting.  items: (pair, y0, x0[, member]), pair an id of add_pair or an (lr, hr)
        tuple of u8 arrays; y0, x0 and the crop size are in LR pixels; member as in step_crops (sr_train_step_pairs_aug)."""
        members = self._members(items)
        arr = (_lib.TrainPairCrop * max(len(items), 1))()
        keep = []
        for k, (pair, y0, x0) in enumerate(it[:3] for it in items):
            it = arr[k]
            it.y0, it.x0 = int(y0), int(x0)
            if isinstance(pair, (int, np.integer)):
                it.pair = int(pair)
            else:
                lr, hr = (np.ascontiguousarray(a) for a in pair)
                if lr.dtype != np.uint8 or hr.dtype != np.uint8 or lr.ndim != 3 or hr.ndim != 3:
                    raise ValueError("expected (h, w, 3|4) u8 pixels")
                it.lh, it.lw = self.engine._pair_shapes(lr.shape, hr.shape)
                keep += [lr, hr]
                it.pair, it.lr_px, it.hr_px = -1, lr.ctypes.data, hr.ctypes.data
                it.lr_channels, it.hr_channels = lr.shape[2], hr.shape[2]
        if members is None:
            rc = self._L.sr_train_step_pairs(self._t, arr, len(items), int(crop_lh), int(crop_lw))
        else:
            rc = self._L.sr_train_step_pairs_aug(self._t, arr, members, len(items), int(crop_lh), int(crop_lw))
        _lib.check(rc, self.engine._ctx)
        self.steps += 1
        self._pending += 1

    def step_pairs(self, lr_batch, hr_batch) -> float:
        """One backprop and one Adam step on a whole batch of pairs: (n,lh,lw,3|4) and (n,f*lh,f*lw,3|4) u8, numpy or torch tensors."""
        lr = lr_batch.cpu().numpy() if hasattr(lr_batch, "cpu") else np.asarray(lr_batch)
        hr = hr_batch.cpu().numpy() if hasattr(hr_batch, "cpu") else np.asarray(hr_batch)
        if lr.ndim == 3 and hr.ndim == 3:
            lr, hr = lr[None], hr[None]
        if lr.shape[0] != hr.shape[0]:
            raise ValueError("expected as many LR as HR images")
        self.step_pair_crops([((lr[i], hr[i]), 0, 0) for i in range(hr.shape[0])], lr.shape[1], lr.shape[2])
        return self.sync()[-1]

    def sync(self) -> List[float]:
        """Wait for every queued step; the err_sum of each step since the last sync."""
        buf = np.empty(max(self._pending, 1), dtype=np.float64)
        n = C.c_size_t()
        _lib.check(self._L.sr_train_sync(self._t, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size, C.byref(n)), self.engine._ctx)
        self._pending = 0
        return [float(v) for v in buf[:n.value]]

    def step(self, hr_batch) -> float:
        """One backprop (loss_scale 1 / n_elems) and one Adam step on a whole batch.  hr_batch: (n,H,W,3|4) u8, numpy or a torch tensor."""
        hr = hr_batch.cpu().numpy() if hasattr(hr_batch, "cpu") else np.asarray(hr_batch)
        if hr.ndim == 3:
            hr = hr[None]
        n, h, w, _ = hr.shape
        self.step_crops([(hr[i], 0, 0) for i in range(n)], h, w)
        return self.sync()[-1]

    def params(self) -> np.ndarray:
        out = np.empty(self.engine.num_params(), dtype=np.float32)
        _lib.check(self._L.sr_train_params(self._t, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), self.engine._ctx)
        return out

    def save(self, path: str):
        """Write the parameters as a .rsr file (bytevec, as the reference's train writes them, main.rs:213)."""
        from . import rsr
        with open(path, "wb") as f:
            f.write(rsr.encode(self.params()))

    def close(self):
        if self._t:
            self._L.sr_train_destroy(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


YuvFormat = _lib.YuvFormat


def yuv_frame_bytes(fmt, h: int, w: int) -> int:
    """sr_yuv_frame_bytes: the bytes of one planar frame of h x w luma samples (0: an invalid format or shape).  Host only."""
    return int(_lib.lib().sr_yuv_frame_bytes(C.byref(fmt), int(h), int(w)))


Yuv16Format = _lib.Yuv16Format


def yuv16_frame_bytes(fmt, h: int, w: int) -> int:
    """sr_yuv16_frame_bytes: the BYTES of one planar frame of h x w 16-bit luma samples (0: an invalid format or shape).  Host only."""
    return int(_lib.lib().sr_yuv16_frame_bytes(C.byref(fmt), int(h), int(w)))


def video_reuse_plan(flags, subsampling, h: int):
    """sr_video_reuse_plan: the LR row bands [(y0, y1), ...] a frame of h luma rows computes, from the row flags of its Y, Cb and Cr
    planes one after another (nonzero: the row differs from the last frame's).  subsampling: "420" | "422" | "444" or the SR_YUV_*
    number.  []: reuse the whole last output; [(0, h)]: the whole frame.  Host only."""
    sub = _lib.Yuv16Format.SUBSAMPLINGS.get(subsampling, subsampling)
    flags = np.ascontiguousarray(flags, dtype=np.uint32).reshape(-1)
    if h >= 1 and sub in (_lib.SR_YUV_420, _lib.SR_YUV_422, _lib.SR_YUV_444) and flags.size != h + 2 * ((h + 1) // 2 if sub == _lib.SR_YUV_420 else h):
        raise ValueError("expected a flag per row of the Y, the Cb and the Cr plane")
    bands, n = (_lib.RowBand * _lib.SR_REUSE_MAX_BANDS)(), C.c_int()
    _lib.check(_lib.lib().sr_video_reuse_plan(flags.ctypes.data_as(C.POINTER(C.c_uint32)), int(sub), int(h), bands, _lib.SR_REUSE_MAX_BANDS, C.byref(n)))
    return [(int(bands[i].y0), int(bands[i].y1)) for i in range(n.value)]


class VideoStream:
    """An sr_video session (include/srhip.h "Video"): frames of h x w in `fmt` go in, frames of fh x fw come out in order, the copies
    of successive frames running under the kernels.  While frames are in flight the engine takes no other call.  `fmt` is a YuvFormat
    or a Yuv16Format (sr_video_create16); either way frames go in and come out as bytes (a u16 array is taken by its bytes).
    reuse=True (sr_video_set_reuse): only the rows a changed input row can reach are computed, the others are the last frame's --
    the frames received are byte for byte the same; reuse_stats() says what that saved.  size=(oh, ow) (sr_video_create*_sized,
    "Video at any size"): the frames come out at that size, the network's f32 output resampled with `filter` (srgb_space: in sRGB
    space) and quantised once; such a session refuses reuse=True with the library's error."""

    def __init__(self, engine: Engine, fmt, h: int, w: int, slots: int = 3, members=None, reuse: bool = False, size=None,
                 filter="lanczos3", srgb_space=False):
        self._L, self._e, self._v = engine._L, engine, C.c_void_p()
        deep = isinstance(fmt, _lib.Yuv16Format)
        frame_bytes, create = (yuv16_frame_bytes, self._L.sr_video_create16) if deep else (yuv_frame_bytes, self._L.sr_video_create)
        self.slots, self.in_bytes = int(slots), frame_bytes(fmt, h, w)
        members = Engine._members(1 if members is None else members)
        if size is None:
            self.out_bytes = frame_bytes(fmt, engine.factor * h, engine.factor * w)
            _lib.check(create(engine._ctx, C.byref(fmt), int(h), int(w), self.slots, members, C.byref(self._v)), engine._ctx)
        else:  # sr_video_create*_sized: the frames come out at size = (oh, ow)
            oh, ow, flt, flags = Engine._resize_args(size, filter, srgb_space)
            create = self._L.sr_video_create16_sized if deep else self._L.sr_video_create_sized
            self.out_bytes = frame_bytes(fmt, oh, ow)
            _lib.check(create(engine._ctx, C.byref(fmt), int(h), int(w), oh, ow, flt, flags, self.slots, members, C.byref(self._v)), engine._ctx)
        if reuse:
            self.set_reuse(True)

    @property
    def pending(self) -> int:
        return int(self._L.sr_video_pending(self._v))

    def set_reuse(self, mode) -> None:
        """sr_video_set_reuse: row reuse on (True / SR_VIDEO_REUSE_ROWS) or off, only with nothing pending; the next frame is whole."""
        _lib.check(self._L.sr_video_set_reuse(self._v, int(mode)), self._e._ctx)

    def reuse_stats(self) -> dict:
        """sr_video_get_reuse_stats as a dict: frames, frames_reused, frames_partial, frames_full, rows_total, rows_computed, bands."""
        st = _lib.VideoReuseStats()
        _lib.check(self._L.sr_video_get_reuse_stats(self._v, C.byref(st)), self._e._ctx)
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def submit(self, frame) -> None:
        """Copy one frame (in_bytes u8) into a free slot's page-locked buffer and queue it; SrError(SR_E_INVALID) if none is free."""
        frame = np.ascontiguousarray(frame)
        frame = (frame if frame.dtype == np.uint16 else frame.astype(np.uint8, copy=False)).reshape(-1).view(np.uint8)
        if frame.size != self.in_bytes:
            raise ValueError(f"expected a frame of {self.in_bytes} bytes")
        p = C.c_void_p()
        _lib.check(self._L.sr_video_acquire(self._v, C.byref(p)), self._e._ctx)
        C.memmove(p, frame.ctypes.data, self.in_bytes)
        _lib.check(self._L.sr_video_submit(self._v), self._e._ctx)

    def receive(self, copy: bool = True) -> np.ndarray:
        """The oldest submitted frame's result (out_bytes u8): copied out of the session's buffer, or with copy=False a view of that
        page-locked buffer, valid until the next receive or close."""
        p = C.c_void_p()
        _lib.check(self._L.sr_video_receive(self._v, C.byref(p)), self._e._ctx)
        view = np.frombuffer((C.c_char * self.out_bytes).from_address(p.value), dtype=np.uint8)
        return view.copy() if copy else view

    def frames(self, iterable):
        """Results of the frames of `iterable`, in order, with the ring kept full."""
        for frame in iterable:
            if self.pending == self.slots:
                yield self.receive()
            self.submit(frame)
        while self.pending > 0:
            yield self.receive()

    def close(self):
        if getattr(self, "_v", None):
            self._L.sr_video_destroy(self._v)
            self._v = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host memory from sr_host_alloc, exposed as a numpy array (`.array`)."""

    def __init__(self, shape, dtype=np.uint8):
        self._L = _lib.lib()
        self._p = C.c_void_p()
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        _lib.check(self._L.sr_host_alloc(C.byref(self._p), nbytes))
        self.array = np.frombuffer((C.c_char * nbytes).from_address(self._p.value), dtype=dtype).reshape(shape)

    def close(self):
        if self._p:
            self.array = None
            self._L.sr_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_alloc(shape, dtype=np.uint8) -> PinnedBuffer:
    return PinnedBuffer(shape, dtype)


class Graph:
    """What `sr_net(FACTOR, None)` returns in the reference (network.rs:16-109),
    reduced to the two methods upscale() uses: num_params() (main.rs:162) and
    forward() (main.rs:171)."""

    def __init__(self, factor: int, device: int = 0):
        if factor not in (2, 3, 4):
            raise _lib.SrError(_lib.SR_E_FACTOR)
        self.factor = factor
        self.device = device
        self._engine: Optional[Engine] = None
        self._params_key = None

    def num_params(self) -> int:
        return _lib.lib().sr_num_params_factor(self.factor)

    def forward(self, n: int, inputs: List[NodeData], params) -> List[NodeData]:
        if len(inputs) != 1:
            raise ValueError("sr_net has exactly one input node")
        p = np.ascontiguousarray(params, dtype=np.float32)
        if p.size != self.num_params():
            raise _lib.SrError(_lib.SR_E_PARAM_COUNT)
        key = (p.size, hash(p.tobytes()))
        if self._engine is None or key != self._params_key:
            if self._engine is not None:
                self._engine.close()
            self._engine = Engine(p, self.device, self.factor)
            self._params_key = key
        inp = inputs[0]
        w, h = inp.shape.spatial_dimensions
        if inp.shape.channels != CHANNELS or inp.shape.n != n:
            raise ValueError("input shape does not match the graph's input node")
        x = np.asarray(inp.values, dtype=np.float32).reshape(n, h, w, CHANNELS)
        out = self._engine.upscale_f32(x)
        return [NodeData(DataShape(CHANNELS, [w * self.factor, h * self.factor], n), out.reshape(-1))]


def bilinear_net(factor: int = FACTOR, device: int = 0) -> "Engine":
    """reference network.rs:111 `pub fn bilinear_net(factor)` (`-p bilinear`): parameter-free."""
    return Engine((), device, factor, graph="bilinear")


def downsample_net(factor: int = FACTOR, device: int = 0) -> "Engine":
    """reference network.rs:125 `pub fn downsample_net(factor)` (`-d`): parameter-free."""
    return Engine((), device, factor, graph="downsample")


def sr_net(factor: int = FACTOR, training=None, device: int = 0) -> Graph:
    """reference network.rs:16 `pub fn sr_net(factor, training)`; inference branch only."""
    if training is not None:
        raise NotImplementedError("training graphs are outside the upscale hot path (SURVEY.md section 8)")
    return Graph(factor, device)
