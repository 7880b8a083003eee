"""Parameter sets and images on which exactly ONE value of exactly one node leaves the domain of the split-half mode -- or, in the
other leg, stays just inside it.  The mode carries every activation as hi + lo / 2048 with hi a half; v_cvt_pkrtz saturates at 65504
silently, so every producer of split values tracks the largest hi it has made and raises the context's domain word
(rusty_sr_amd/csrc/sr_kernels.hip domain_track / domain_report; include/srhip.h sr_check_domain).  The rest of the suite trips that
check through a poisoned input value or an f_bias of 7e4 on every channel of every pixel; here the offending value is one channel
of one pixel of the node of our choice, so each stage epilogue, tile class, lane and plan has to find it on its own.

A case is (node X, pixel P, channel b) and a leg.  The parameters are "wired" from a base set (imagenet.rsr at factor 3,
param_families.bundled_scale at factors 2 and 4):

  into X     X != f: channel A of conv0 is the centre tap from R alone (gain 50), f_bias[A] = 0, f_activ[A] = 1, and channel b of X's
             convolution over f (conv1 / conv2 / conv3) is the centre tap from f's channel A alone, gain g.  X == f: the centre tap of
             conv0 from R into channel b carries g.  X_bias[b] = 0, X_activ[b] = 1.
  out of X   every later convolution that feeds a split node reads nothing from channel b of X (conv1 / 2 / 3 for f, conv5 / 6 for
             l1, conv8 for l2); the expand convolutions (conv7, conv9, conv10) keep reading it, so the output depends on the value.
  image      a dark picture (synth_u8 // 8) with R = 255 at P.
  g          by a bracketing search (bisection, cut where the chord meets the target) on the f64 oracle, so that max|X| is 0.97 x 65504 (leg "under") or 1.03 x 65504 (leg "over").  The GPU's
             node error is below 1e-6 relative (profiles/param_families_errors.txt): the 3 % margin is tens of thousands of it.

The input-boundary cases need no bisection: an f32 image of small values with one sample at 65504, -65504 or the float just below
65504 (which cvt_pkrtz takes to 0x7bfe), on the `dim` family (conv0 and f_bias at 1e-3 of scale, so node f stays small).

No GPU here: tests/test_domain_cases_cpu.py proves on the oracle alone that every case is what it claims;
tests/test_gpu_domain_nodes.py runs them through the kernels."""
import numpy as np

import grad_ref
import oracle
import param_families as pf
from conftest import synth_u8

LIMIT = 65504.0                 # the largest half: a hi half of 0x7bff raises the flag
H, W = 37, 75                   # the ragged shape of param_families.image("synth"): partial tiles on both axes
NODES = pf.NODES
A = 5                           # the channel of f that carries the bright pixel into l1 / l2 / l3
R_GAIN = 50.0
CHANNELS = (0, 31)
LEGS = {"under": 0.97, "over": 1.03}
OTHERS_BAR = 0.25               # every other split value stays below this share of the limit (a condition; the cases reach 0.093)
F_CONV = {"l1": "conv1", "l2": "conv2", "l3": "conv3"}
SPLIT_READERS = {"f": ("conv1", "conv2", "conv3"), "l1": ("conv5", "conv6"), "l2": ("conv8",), "l3": ()}
EXPAND_READER = {"l1": "conv7", "l2": "conv9", "l3": "conv10"}
# (0, 0), the last pixel, and an interior pixel on a tile seam: row 15 ends an 8-row tile and a 4-row tile, column 32 begins a tile
POSITIONS = {"first": (0, 0), "last": (H - 1, W - 1), "seam": (15, 32)}
OUT_TOL = 1e-4                  # the project's rule for large values: |gpu - want| <= 1e-4 max|want| (tests/test_gpu_domain.py)


def base_params(factor):
    return pf.weights("imagenet", 3) if factor == 3 else pf.bundled_scale(factor, pf.seed_of(factor))


def _view(p, factor, name):
    off, n, shape = grad_ref.segments(factor)[name]
    return p[off:off + n].reshape(shape)


def wired(node, b, g, factor=3):
    """the base parameters of `factor` with the one path of gain g into channel b of `node`, and nothing split reading it"""
    p = np.array(base_params(factor), dtype=np.float32, copy=True)
    if node == "f":
        c0 = _view(p, factor, "conv0")
        c0[b] = 0
        c0[b, 2, 2, 0] = g
    else:
        c0 = _view(p, factor, "conv0")
        c0[A] = 0
        c0[A, 2, 2, 0] = R_GAIN
        _view(p, factor, "f_bias")[A] = 0
        _view(p, factor, "f_activ")[A] = 1
        cx = _view(p, factor, F_CONV[node])
        cx[b] = 0
        cx[b, 2, 2, A] = g
    _view(p, factor, node + "_bias")[b] = 0
    _view(p, factor, node + "_activ")[b] = 1
    for name in SPLIT_READERS[node]:
        _view(p, factor, name)[:, :, :, b] = 0
    return p


def image_u8(pos, seed=0):
    """(1, H, W, 3) u8: dark, R = 255 at POSITIONS[pos]"""
    px = synth_u8(900 + seed, 1, H, W) // 8
    y, x = POSITIONS[pos]
    px[0, y, x, 0] = 255
    return np.ascontiguousarray(px.astype(np.uint8))


def nodes_f64(p, x, factor=3):
    """{node: (H, W, 32) f64} of the oracle.  forward_taps is sr_net(3)'s; the nodes f .. l3 of the other factors are the same function
    of the segments every factor has (only the expand convolutions and their bias differ in size), so those are copied into a
    factor-3 parameter vector whose expand part is zero."""
    return _taps(p, x, factor, True)


def _taps(p, x, factor, f64):
    if factor != 3:
        q = np.zeros(oracle.NPARAMS, dtype=np.float32)
        for name, (off, n, shape) in grad_ref.segments(factor).items():
            if shape[0] == 32:
                o3 = oracle.SEGMENTS[name][0]
                q[o3:o3 + n] = p[off:off + n]
        p = q
    _, t = oracle.forward_taps(p, x, f64=f64)
    return {k: t[k] for k in NODES}


def _peak(node, b, g, x, factor):
    return float(np.abs(nodes_f64(wired(node, b, g, factor), x, factor)[node]).max())


def find_gain(node, b, x, target, factor=3):
    """the float32 g at which max|node| of the f64 oracle is `target`, by bisection of a bracket (the peak grows with g: BeLU with beta 1 is
    increasing, and the path into it is one product).  Ends when the peak is within 1e-4 of the target, a thirtieth of the margin
    between the legs and the limit itself."""
    lo, hi = 0.0, 1.0
    vlo, vhi = _peak(node, b, lo, x, factor), _peak(node, b, hi, x, factor)
    while vhi < target:
        lo, vlo = hi, vhi
        hi *= 16.0
        assert hi < 1e9
        vhi = _peak(node, b, hi, x, factor)
    for k in range(60):
        # the bracket is cut where the chord meets the target (the peak is all but linear in g once it sits at P), and every third
        # time in the middle, which alone guarantees the end
        cut = 0.5 if k % 3 == 2 else min(max((target - vlo) / (vhi - vlo), 0.0), 1.0)
        mid = float(np.float32(lo + cut * (hi - lo)))
        v = _peak(node, b, mid, x, factor)
        if abs(v - target) <= 1e-4 * target:
            return mid
        if v < target:
            lo, vlo = mid, v
        else:
            hi, vhi = mid, v
    raise AssertionError((node, b, target, lo, hi))


class Case:
    """One (node, position, channel, leg, factor): .params, .px (u8), .x (f32), and the oracle's .t64 (nodes), .o64, .o32 (outputs)."""

    def __init__(self, node, pos, b, leg, factor=3):
        self.node, self.pos, self.b, self.leg, self.factor = node, pos, b, leg, factor
        self.px = image_u8(pos)
        self.x = oracle.img_to_data(self.px)
        self.g = find_gain(node, b, self.x, LEGS[leg] * LIMIT, factor)
        self.params = wired(node, b, self.g, factor)
        for a in (self.px, self.x, self.params):
            a.flags.writeable = False
        self._truth = None

    @property
    def P(self):
        return POSITIONS[self.pos]

    @property
    def id(self):
        return f"{self.node}-{self.pos}-b{self.b}-{self.leg}" + ("" if self.factor == 3 else f"-f{self.factor}")

    def _run(self):
        if self._truth is None:
            t64 = nodes_f64(self.params, self.x, self.factor)
            t32 = _taps(self.params, self.x, self.factor, False)
            o64 = oracle.forward_factor(self.params, self.x, self.factor, f64=True)
            o32 = oracle.forward_factor(self.params, self.x, self.factor)
            for a in list(t64.values()) + list(t32.values()) + [o64, o32]:
                a.flags.writeable = False
            self._truth = (t64, t32, o64, o32)
        return self._truth

    t64 = property(lambda self: self._run()[0])
    t32 = property(lambda self: self._run()[1])
    o64 = property(lambda self: self._run()[2])
    o32 = property(lambda self: self._run()[3])


_CASES = {}


def case(node, pos, b, leg, factor=3):
    """the one Case of these coordinates: built once (its bisection and its oracle runs), shared and left unchanged"""
    key = (node, pos, b, leg, factor)
    if key not in _CASES:
        _CASES[key] = Case(*key)
    return _CASES[key]


# every (node, position, channel) at factor 3, and l3 once at each of the other factors
TABLE = [(node, pos, b, 3) for node in NODES for pos in POSITIONS for b in CHANNELS] + [("l3", "seam", 31, 2), ("l3", "last", 0, 4)]


def table_id(row):
    node, pos, b, factor = row
    return f"{node}-{pos}-b{b}" + ("" if factor == 3 else f"-f{factor}")


def expand_of_channel(c, dmap):
    """What the f64 output of case c (node != f) changes by when channel b of c.node changes by the (H, W) map `dmap`: the expand
    convolution that reads the node is the only reader left (3x3, zero padding: e[y, x, o] = sum w[o, ky, kx, i] X[y + ky - 1,
    x + kx - 1, i]), and Expand sends channel (dy f + dx) 3 + ch of pixel (y, x) to out[f y + dy, f x + dx, ch].  -> (f H, f W, 3)
    f64.  (tests/test_domain_cases_cpu.py checks this restatement against the oracle: the over leg's output minus the under leg's.)"""
    f = c.factor
    w = _view(np.asarray(c.params), f, EXPAND_READER[c.node]).astype(np.float64)
    pad = np.pad(np.asarray(dmap, dtype=np.float64), 1)
    e = np.zeros((H, W, 3 * f * f))
    for ky in range(3):
        for kx in range(3):
            e += pad[ky:ky + H, kx:kx + W, None] * w[None, None, :, ky, kx, c.b]
    return e.reshape(H, W, f, f, 3).transpose(0, 2, 1, 3, 4).reshape(f * H, f * W, 3)


def saturated_output_error(c):
    """max |output with c.node[P, b] replaced by +-65504 - the true output| in f64: what a kernel that clamped silently would be off by"""
    y, x = c.P
    v = float(c.t64[c.node][y, x, c.b])
    dmap = np.zeros((H, W))
    dmap[y, x] = np.copysign(LIMIT, v) - v
    return float(np.abs(expand_of_channel(c, dmap)).max())


# ---- the input-boundary cases ----------------------------------------------------------------------------------------------------------
BELOW = float(np.nextafter(np.float32(LIMIT), np.float32(0)))     # 65503.996: rounds toward zero to 0x7bfe (65472)
BOUNDARY = {"at": (LIMIT, True), "minus": (-LIMIT, True), "below": (BELOW, False)}    # name -> (the sample, whether it leaves the domain)
BOUNDARY_AT = (15, 32, 1)       # the seam pixel's G


def boundary_params():
    return pf.weights("dim", 3)


def boundary_image(which):
    """(1, H, W, 3) f32 in [0, 0.25) with the one sample"""
    x = (np.random.default_rng(77).random((1, H, W, 3), dtype=np.float32) * np.float32(0.25)).astype(np.float32)
    y, xx, ch = BOUNDARY_AT
    x[0, y, xx, ch] = np.float32(BOUNDARY[which][0])
    return x
