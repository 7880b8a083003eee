"""The multi-round paths of the aux and scoring kernels, against their references.

Every kernel here walks more than one piece of work per workgroup once its input is large enough -- a grid stride with the next piece
prefetched (sr_aux.hip), a capped grid (valid_loss_kernel), rounds of 256 partials (loss_sum_kernel, metrics_sum_kernel), capped chunk
counts (sr_grad.hip layout()) -- and the other files compare them with a reference only where each workgroup does one piece.  Here:
 a. the aux graphs under sr_set_experiment "auxgrid" (a cap on the workgroup count: the kernels take their stride from gridDim.x),
    at tiny shapes, against the oracle, and bit-identical to the uncapped call;
 b. the aux graphs' automatic grid at frame sizes where it strides on its own;
 c. the validation loss beyond 256 partials and beyond one round of its capped grid, against the f64 restatement;
 d. the metrics beyond 256 tiles, against tests/metrics_ref.py;
 e. the backward pass across its chunk caps: a batch against the f64 sum of its images' gradients.
The bars are those of the tests these shapes extend (test_bilinear_and_downsample_graphs, test_reduction_is_exact,
test_gpu_metrics.accept, assert_grad_close, test_batch_is_the_sum_of_its_images)."""
import functools
import math

import numpy as np
import pytest
import torch

import metrics_ref
import oracle
from conftest import synth_u8
from test_gpu_backprop import assert_grad_close, hr_batch
from test_gpu_metrics import accept, noisy, with_channels
from test_gpu_parity import _check_u8
from test_gpu_validation import err_of, hr_image, synthetic_params

pytestmark = pytest.mark.gpu

F32_BAR = 1e-5   # max |gpu - oracle| of the f32 aux graphs (test_bilinear_and_downsample_graphs)


@pytest.fixture(scope="module")
def aux():
    import rusty_sr_amd as r
    e = {"bilinear": r.bilinear_net(r.FACTOR), "downsample": r.downsample_net(r.FACTOR)}
    yield e
    for x in e.values():
        x.close()


def _make_case(graph, n, h, w, ch):
    """(u8 pixels with ch channels, the f32 image of their colours, the oracle's output), none of them writable."""
    px = synth_u8(7000 + 13 * h + w, n, h, w)
    x = oracle.img_to_data(px)
    want = oracle.bilinear(x) if graph == "bilinear" else oracle.downsample(x)
    if ch == 4:
        px = np.concatenate([px, synth_u8(7500 + 13 * h + w, n, h, w)[..., :1]], axis=-1)  # an alpha channel nobody reads
    for a in (px, x, want):
        a.setflags(write=False)
    return px, x, want


_aux_case = functools.lru_cache(maxsize=None)(_make_case)   # the small shapes: made once, shared by the tests and caps that use them


def _at_offset(px, off):
    """The pixels in device memory, their first byte `off` bytes behind a 4-byte aligned address."""
    buf = torch.zeros(px.size + 8, dtype=torch.uint8, device="cuda")
    view = buf[off:off + px.size].view(px.shape)
    view.copy_(torch.from_numpy(np.array(px)))
    assert view.data_ptr() % 4 == off and view.is_contiguous()
    return view


def _strided(eng, graph, img, ch, cap, what):
    """Every launch of the last call is on the record, walked more pieces than it had workgroups, and kept to the cap."""
    rec = eng.last_plan()["aux"]
    assert rec, (what, eng.get_experiment("plan"))
    for l in rec:
        assert (l["graph"], l["img"], l["ch"]) == (graph, img, ch), (what, l)
        assert l["units"] > l["grid"] >= 1, f"{what}: this launch did not stride: {l}"
        assert cap is None or l["grid"] <= cap, (what, l)
    return rec


def _out_shape(eng, n, h, w, c):
    return (n,) + eng._out_hw(h, w) + (c,)


def _run(eng, graph, img, ch, caps, calls, check, what0):
    """calls: name -> (poison, call).  poison() leaves wrong values wherever call() is about to write -- a piece that a strided launch
    skips must not find the right bytes of an earlier call of the same shape still there; it always runs on the automatic grid."""
    def measured(name, cap):
        poison, call = calls[name]
        eng.set_experiment("auxgrid", "")
        poison()
        eng.set_experiment("auxgrid", cap)
        return call()
    try:
        plain = {}
        for name in calls:
            plain[name] = measured(name, "")
            rec = eng.last_plan()["aux"]
            check(plain[name], what0 + ("", name))
            assert len(rec) == 1 and rec[0]["count"] == 1, (what0, name, rec)  # one chunk, one launch: on the record without the switch too
        for cap in caps:
            for name in calls:
                what = what0 + (cap, name)
                got = measured(name, str(cap))
                _strided(eng, graph, img, ch, cap, what)
                check(got, what)
                np.testing.assert_array_equal(got, plain[name], err_msg=str(what))
    finally:
        eng.set_experiment("auxgrid", "")


def _run_u8(eng, graph, n, h, w, ch, caps, offset1):
    """One u8 shape through the host and the device entry point (and from a device pointer at byte 1), uncapped and under every cap."""
    px, _, want = _aux_case(graph, n, h, w, ch)
    other = 255 - px   # the host calls' poison: another image through the same staging buffers
    calls = {"host": (lambda: eng.upscale_rgba8(other), lambda: eng.upscale_rgba8(px))}
    for off in ((0, 1) if offset1 else (0,)):
        view, out = _at_offset(px, off), torch.empty(_out_shape(eng, n, h, w, 4), dtype=torch.uint8, device="cuda")
        calls[f"dev+{off}"] = (lambda out=out: out.fill_(0x5A), lambda view=view, out=out: eng.upscale_rgba8_dev(view, out=out).cpu().numpy())
    _run(eng, graph, "u8", ch, caps, calls, lambda got, what: _check_u8(got, want), (graph, "u8", n, h, w, ch))


def _run_f32(eng, graph, n, h, w, caps):
    _, x, want = _aux_case(graph, n, h, w, 3)
    other = 1.0 - x
    xd, out = torch.from_numpy(np.array(x)).cuda(), torch.empty(_out_shape(eng, n, h, w, 3), dtype=torch.float32, device="cuda")
    calls = {"host": (lambda: eng.upscale_f32(other), lambda: eng.upscale_f32(x)),
             "dev": (lambda: out.fill_(float("nan")), lambda: eng.upscale_f32_dev(xd, out=out).cpu().numpy())}

    def check(got, what):
        assert got.shape == want.shape, what
        err = float(np.abs(got - want).max())
        print(f"{what}: max |gpu - oracle| = {err:.3e}")
        assert err < F32_BAR, (what, err)
    _run(eng, graph, "f32", 3, caps, calls, check, (graph, "f32", n, h, w))


# ---- a. capped grids at small shapes ----------------------------------------------------------------------------------------
# bilinear_u8_kernel: a wave's item is (image n, input row y, block b of 64 chunks), nb = ceil(ceil(3 W / 4) / 64) blocks per row, and
# a wave steps nw = 4 x grid items at a time through (n, y, b) as a mixed-radix counter.
U8_BILINEAR = [  # (n, H, W, ch, auxgrid, also from a device pointer at byte 1)
    (5, 2, 20, 3, 1, False),    # nb 1: nw = 4 >= nb H, the image index jumps by 2
    (3, 3, 100, 4, 1, False),   # nb 2: y carries into n
    (2, 5, 400, 3, 1, False),   # nb 5: nw < nb, b carries into y on every step
    (2, 5, 400, 3, 2, True),    # nb 5: mixed steps
    (2, 5, 400, 3, 3, False),
    (2, 7, 401, 4, 2, True),    # W % 4 != 0: the dword-store form
    (1, 9, 2, 3, 1, False),     # W < 3: the byte-wise window
]


@pytest.mark.parametrize("n,h,w,ch,cap,offset1", U8_BILINEAR)
def test_u8_bilinear_under_a_capped_grid(aux, n, h, w, ch, cap, offset1):
    _run_u8(aux["bilinear"], "bilinear", n, h, w, ch, [cap], offset1)


# bilinear_tile_kernel: tiles of 64 x 16 input pixels, the next tile's pixels fetched one round ahead
F32_BILINEAR = [  # (n, H, W, caps)
    (2, 33, 130, (1, 4, 5)),   # 18 tiles, W % 4 != 0; with 5 workgroups the last round is partial: the prefetch's guard
    (1, 17, 132, (1, 4)),      # 6 tiles, the 16-byte-store form
    (3, 1, 1, (2,)),           # 3 tiles of one pixel
]


@pytest.mark.parametrize("n,h,w,caps", F32_BILINEAR)
def test_f32_bilinear_under_a_capped_grid(aux, n, h, w, caps):
    _run_f32(aux["bilinear"], "bilinear", n, h, w, caps)


# downsample_tile_kernel: tiles of 64 x 4 outputs (192 x 12 inputs), the next tile's windows fetched one round ahead
DOWNSAMPLE = [  # (n, H, W, ch of the u8 form, caps)
    (2, 40, 400, 3, (1, 5, 7)),   # 24 tiles
    (1, 37, 200, 4, (4,)),        # 6 tiles
]


@pytest.mark.parametrize("n,h,w,ch,caps", DOWNSAMPLE)
def test_u8_downsample_under_a_capped_grid(aux, n, h, w, ch, caps):
    _run_u8(aux["downsample"], "downsample", n, h, w, ch, caps, offset1=True)


@pytest.mark.parametrize("n,h,w,ch,caps", DOWNSAMPLE)
def test_f32_downsample_under_a_capped_grid(aux, n, h, w, ch, caps):
    _run_f32(aux["downsample"], "downsample", n, h, w, caps)


def test_auxgrid_takes_a_positive_integer_or_nothing(aux):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    eng = aux["bilinear"]
    px, _, _ = _aux_case("bilinear", 2, 5, 400, 3)
    try:
        for bad in ("0", "-1", "x", "3x", " 3", "1.5", "+2", "99999999999"):
            with pytest.raises(r.SrError) as ex:
                eng.set_experiment("auxgrid", bad)
            assert ex.value.status == _lib.SR_E_INVALID, bad
        eng.set_experiment("auxgrid", "3")
        with pytest.raises(r.SrError):   # a refused value leaves the switch as it was
            eng.set_experiment("auxgrid", "0")
        eng.upscale_rgba8(px)
        assert [l["grid"] for l in eng.last_plan()["aux"]] == [3]
        eng.set_experiment("auxgrid", "1000000")   # a cap above the automatic grid changes nothing
        eng.upscale_rgba8(px)
        capped = eng.last_plan()["aux"]
        eng.set_experiment("auxgrid", "")
        eng.upscale_rgba8(px)
        assert eng.last_plan()["aux"] == capped and capped[0]["units"] == 13  # 2 x 5 x 5 items in fours
    finally:
        eng.set_experiment("auxgrid", "")


# ---- b. the automatic grid, where it strides on its own ---------------------------------------------------------------------
@pytest.mark.parametrize("graph,h,w,ch", [("bilinear", 720, 1280, 3), ("bilinear", 721, 1281, 4), ("downsample", 2160, 3840, 3)])
def test_u8_frames_stride_on_the_automatic_grid(aux, graph, h, w, ch):
    """Device entry points: one call is one launch.  A launch that does not stride on this machine fails the test, naming the shape."""
    eng = aux[graph]
    px, _, want = _make_case(graph, 1, h, w, ch)
    out = torch.full(_out_shape(eng, 1, h, w, 4), 0x5A, dtype=torch.uint8, device="cuda")   # (a piece left out keeps these bytes)
    got = eng.upscale_rgba8_dev(torch.from_numpy(np.array(px)).cuda(), out=out).cpu().numpy()
    rec = _strided(eng, graph, "u8", ch, None, f"{graph} {w} x {h} ch {ch} on the automatic grid")
    assert len(rec) == 1 and rec[0]["count"] == 1, rec
    _check_u8(got, want)


# ---- c. the validation loss beyond one round --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng2():
    import rusty_sr_amd as r
    e = r.Engine(synthetic_params(2, 102), device=0, factor=2)
    yield e
    e.close()


VALID = [  # (kind, HR h, HR w, linear loss)
    # 514 x 512 = 263 168 px = 65 792 items of 4 px = 257 workgroups: loss_sum_kernel's second round of 256 partials
    ("u8_4", 514, 512, False),
    ("f32", 514, 512, True),
    # valid_loss_kernel's grid is capped at 2048 workgroups x 256 threads x 4 px = 2 097 152 px; 1450 x 1450 = 2 102 500 px goes 5 348
    # px into its second stride round, and 1450 % 4 = 2 puts a row seam into every other item row
    ("u8_3", 1450, 1450, False),
    ("f32", 1450, 1450, True),
]


@pytest.mark.parametrize("kind,h,w,linear", VALID)
def test_validation_loss_beyond_one_round(eng2, kind, h, w, linear):
    hr = hr_image(kind, h, w, 31 * h + w)
    err, n = eng2.validation_error(hr, linear_loss=linear)
    _, out = eng2.validation_nodes(h, w)
    want, m = err_of(out, hr, 2, linear)
    assert n == m == 3 * h * w
    print(f"{(kind, h, w, linear)}: gpu {err!r} restatement {want!r} rel {abs(err - want) / want:.3e}")
    assert err == pytest.approx(want, rel=1e-12), (kind, err, want)


# ---- d. metrics with more than 256 tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,shave,ca,cb", [(24, 8300, 0, 3, 4), (24, 8300, 3, 4, 3), (8300, 24, 0, 4, 4)])
def test_metrics_beyond_256_tiles(eng2, h, w, shave, ca, cb):
    """260 tiles of 32 in one row (one column) of tiles: metrics_sum_kernel's second round of 256 partials."""
    from rusty_sr_amd import _lib
    tiles = -(-(h - 2 * shave) // _lib.SR_METRICS_TILE) * -(-(w - 2 * shave) // _lib.SR_METRICS_TILE)
    assert tiles == 260
    base = synth_u8(600 + h + shave, 1, h, w)[0]
    a, b = with_channels(noisy(base, 601 + shave), ca, 1), with_channels(base, cb, 2)
    accept(eng2.image_metrics(a, b, shave=shave), metrics_ref.metrics(a, b, shave), (h, w, shave, ca, cb))


# ---- e. the backward pass across its chunk caps, by additivity --------------------------------------------------------------
# layout() (sr_grad.hip): min(128, ceil(LR px / 512)) weight-gradient chunks, min(256, ceil(LR px / 1024)) column-sum chunks.  A single
# image of a case stays below the cap the case is about, the batch is past it: its gradient must be the sum of its images', which no
# autograd run at these sizes is needed for.  loss_scale 1: the default depends on the element count.
@pytest.mark.parametrize("kind,n,side,lr_px,cap", [
    ("u8_3", 2, 400, 80_000, 65_536),      # 2 x 40 000 LR px: wchunks capped at 128 (from 65 536 on), chunks of 625
    ("u8_4", 4, 530, 280_900, 262_144),    # 4 x 70 225 LR px: cchunks capped at 256 (from 262 144 on) as well
])
def test_backward_pass_across_its_chunk_caps(eng2, kind, n, side, lr_px, cap):
    p = synthetic_params(2, 102)
    assert n * (side // 2) ** 2 == lr_px > cap >= (side // 2) ** 2
    hr = hr_batch(kind, n, side, side, 77 + side)
    err, ne, g = eng2.backprop(hr, p, loss_scale=1.0)
    parts = [eng2.backprop(hr[i:i + 1], p, loss_scale=1.0) for i in range(n)]
    assert ne == sum(q[1] for q in parts) == n * 3 * side * side
    want_err = math.fsum(q[0] for q in parts)
    print(f"err_sum {err!r} sum of images {want_err!r}")
    assert abs(err - want_err) <= 1e-9 * err
    assert np.isfinite(g).all()
    assert_grad_close(g, sum(q[2].astype(np.float64) for q in parts), 2, (kind, n, side))
