"""The stage kernels at the edges of the index space and of buffer placement, each call followed by an assertion on what it ran (the
plan record, Engine.last_plan).

1. Tall, thin images: 1-33 columns (one or two tile columns, 28-31 padding columns in a tile) of 1-2001 rows, and 8200 rows (more
   than two rounds of 8-row tiles in one tile column), at factors 2-4, through the host and device entry points in every final-stage
   form; the forked device call at its minimum heights.
2. Wide strips: 1-9 rows of 32 767 to 100 003 columns (thousands of tile columns, output rows of 300 000 pixels).
3. Many tiny images: batches of 1000-4096 images of 1x1 to 5x7 pixels, and a batch larger than one host chunk.
4. Planner corners: frames at every threshold of plan_chunks, its smallest three-band plan (bands of 8 rows), the forced band plans at
   2 x SR_HALO rows and at a single own row, and the band entry points at one own row.
5. Buffer placement and streams: inputs and outputs that start inside a larger allocation, calls on a side stream, and the 4-byte
   alignment the device entry points require of RGBA and f32 buffers.

The oracle checks follow tests/test_gpu_kernel_matrix.py: f32 output against the C oracle and its f64 leg, u8 output equal to the
quantised f32 output bit for bit, RGBA input with a random alpha plane equal to the RGB result.  Everything else is bit for bit
against the undivided device call of the same context."""
import ctypes as C

import numpy as np
import pytest

import oracle
from conftest import synth_u8
from test_gpu_kernel_matrix import FORMS, SWITCHES, TOL, _cell_of, _check_u8, _quantise, _synthetic_params, \
    _with_alpha

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
SR_HALO = 7


@pytest.fixture(scope="module")
def weights(params):
    return {2: _synthetic_params(2, 102), 3: params["imagenet"], 4: _synthetic_params(4, 104)}


@pytest.fixture(scope="module")
def engines(weights):
    """One context per (factor, precision), shared by the whole module."""
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision):
        if (factor, precision) not in made:
            made[(factor, precision)] = r.Engine(weights[factor], device=0, factor=factor, precision=precision)
        e = made[(factor, precision)]
        _reset(e)
        return e
    yield get
    for e in made.values():
        e.close()


_ORACLE = {}


def _truth(weights, factor, name, x, f64=True):
    """One oracle run (f32, and f64 where asked) per (factor, image), shared by both precisions, every form and entry point."""
    key = (factor, name)
    if key not in _ORACLE:
        _ORACLE[key] = (oracle.forward_factor(weights[factor], x, factor),
                        oracle.forward_factor(weights[factor], x, factor, f64=True) if f64 else None)
    return _ORACLE[key]


def _reset(eng):
    for k in SWITCHES + ("bands", "rows"):
        eng.set_experiment(k, "")
    eng.set_pipeline(True)


def _finals(eng):
    return [l for l in eng.last_plan()["launches"] if l["st"] == 4]


def _expect_final(eng, form, factor, precision, img, out, ch):
    """Every final-stage launch of the last call ran `form` (a FORMS key, or "first" / "pipe" for the form alone) on this I/O."""
    fin = _finals(eng)
    assert fin, eng.get_experiment("plan")
    for l in fin:
        assert (l["f"], l["prec"], l["img"], l["out"], l["ch"]) == (factor, precision, img, out, ch), l
        if "/" in form:
            want = form
            if precision == "split_f16" and factor == 4:
                want = form.split("/")[0] + "/4"   # kBigTiles: the 4-row body only (sr_kernels.hip)
            assert _cell_of(l) == want, (form, eng.get_experiment("plan"))
        else:
            assert l["form"] == form, (form, eng.get_experiment("plan"))
    return _cell_of(fin[0])


def _force(eng, form):
    _reset(eng)
    if "/" in form:
        for k, v in FORMS[form].items():
            eng.set_experiment(k, v)
    else:
        eng.set_experiment("pipe", "none" if form == "first" else "all")


def _host_rec(eng):
    rec = eng.last_plan()["host"]
    assert len(rec) == 1, rec
    return rec[0]


COVERAGE = {}  # section -> {cell: set of what was asserted}


def _cover(section, cell, what):
    COVERAGE.setdefault(section, {}).setdefault(cell, set()).add(what)


F64_FLOOR = 2e-7   # the CPU f32 path's error against f64 taken as at least this (3-4 ulp of an output near 0.5-1), see _check


def _check(got, want32, want64, tol):
    """_check_f32's two bounds: against the f32 oracle, and against exact arithmetic (the f64 leg) as close as the CPU f32 path is,
    that path's largest error counted as at least F64_FLOOR.  (An image of a few pixels is a small sample: there the CPU's largest
    error can be a single ulp by chance, and the GPU's different summation order a few.)  Without the f64 leg (large images): the
    f32 bound alone."""
    assert got.shape == want32.shape
    assert np.abs(got - want32).max() < tol
    if want64 is not None:
        cpu = max(np.abs(want32.astype(np.float64) - want64).max(), F64_FLOOR)
        assert np.abs(got.astype(np.float64) - want64).max() <= 2 * cpu + 1e-7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. tall, thin images ------------------------------------------------------------------------------------------------------------

THIN_W = (1, 2, 3, 4, 31, 32, 33)
THIN_H = (1, 7, 8, 9, 300, 2001)
LONG_H = 8200   # 1025 8-row tiles per tile column: more than two rounds of them (512 per round on 256 CUs), the mixed cell reachable
LONG_W = (1, 32, 33)


def _thin_cell(eng, form, factor, precision, px, x, want32, want64, tol, seed):
    """Host and device entry points, f32 / u8 / RGBA, in one forced form."""
    import torch
    _force(eng, form)
    eng.set_pipeline(False)   # one chunk: the forced switches apply to the one launch of each stage
    got32 = eng.upscale_f32(x)
    cell = _expect_final(eng, form, factor, precision, "f32", "f32", 3)
    assert [k for k, _, _ in eng.last_plan()["host"]] == ["one"]
    _check(got32, want32, want64, tol)
    got8 = eng.upscale_rgba8(px)
    _expect_final(eng, form, factor, precision, "u8", "u8", 3)
    np.testing.assert_array_equal(got8, _quantise(got32), err_msg=f"host u8 != quantised f32 ({form})")
    _check_u8(got8, want32)
    np.testing.assert_array_equal(eng.upscale_rgba8(_with_alpha(px, seed)), got8, err_msg=f"host RGBA != RGB ({form})")
    _expect_final(eng, form, factor, precision, "u8", "u8", 4)
    eng.set_experiment("fork", "0")
    d32 = eng.upscale_f32_dev(_dev(x)).cpu().numpy()
    _expect_final(eng, form, factor, precision, "f32", "f32", 3)
    _check(d32, want32, want64, tol)
    d8 = eng.upscale_rgba8_dev(_dev(px)).cpu().numpy()
    _expect_final(eng, form, factor, precision, "u8", "u8", 3)
    np.testing.assert_array_equal(d8, _quantise(d32), err_msg=f"device u8 != quantised f32 ({form})")
    d8a = eng.upscale_rgba8_dev(_dev(_with_alpha(px, seed + 1))).cpu().numpy()
    _expect_final(eng, form, factor, precision, "u8", "u8", 4)
    np.testing.assert_array_equal(d8a, d8, err_msg=f"device RGBA != RGB ({form})")
    torch.cuda.synchronize()
    return cell


@pytest.mark.parametrize("factor", [2, 3, 4])
def test_tall_thin_images_against_the_oracle(weights, engines, factor):
    shapes = [(h, w) for w in THIN_W for h in THIN_H] + [(LONG_H, w) for w in LONG_W]
    for (h, w) in shapes:
        px = synth_u8(1000 * factor + 10 * w + h % 10, 1, h, w)
        x = oracle.img_to_data(px)
        want32, want64 = _truth(weights, factor, f"thin{h}x{w}", x)
        for precision in PRECISIONS:
            eng = engines(factor, precision)
            for form in ("first/4", "first/8", "pipe/4", "pipe/8") + (("pipe/8+4",) if h == LONG_H else ()):
                try:
                    cell = _thin_cell(eng, form, factor, precision, px, x, want32, want64, TOL, seed=h + w)
                except AssertionError as e:
                    raise AssertionError(f"{h}x{w} f{factor} {precision} {form}: {e}") from e
                _cover("1 tall thin", f"{precision} f{factor}", cell)
            _reset(eng)


@pytest.mark.parametrize("factor", [2, 3, 4])
def test_forked_tall_thin_images_at_their_minimum_heights(engines, factor):
    """The fork needs own >= 4 SR_HALO rows and keeps >= 2 SR_HALO rows in each band: own = 28 (one cut), 29 and 36, one or two
    columns; the planned cut ("1") and every explicit first band the clamp allows at the ends -- bit-identical to "fork" = "0"."""
    import torch
    rng = np.random.default_rng(70 + factor)
    for precision in PRECISIONS:
        eng = engines(factor, precision)
        for w in (1, 2):
            for own in (28, 29, 36):
                px = rng.integers(0, 256, (own, w, 3), dtype=np.uint8)
                d8, d32 = _dev(px[None]), _dev(oracle.img_to_data(px)[None])
                eng.set_experiment("fork", "0")
                want8, want32 = eng.upscale_rgba8_dev(d8), eng.upscale_f32_dev(d32)
                assert eng.last_plan()["fork"] == [(False, 0, 0)]
                for cut in ("1", str(2 * SR_HALO), str(own - 2 * SR_HALO), str(own // 2)):
                    eng.set_experiment("fork", cut)
                    got8 = eng.upscale_rgba8_dev(d8)
                    rec8 = eng.last_plan()["fork"]
                    got32 = eng.upscale_f32_dev(d32)
                    rec32 = eng.last_plan()["fork"]
                    for rec in (rec8, rec32):
                        assert len(rec) == 1 and rec[0][0] and rec[0][1] + rec[0][2] == own, (own, cut, rec)
                        assert min(rec[0][1], rec[0][2]) >= 2 * SR_HALO, rec
                        if cut != "1":
                            assert rec[0][1] == int(cut), (cut, rec)
                    assert torch.equal(got8, want8), (precision, w, own, cut)
                    assert torch.equal(got32, want32), (precision, w, own, cut)
                    _cover("1 fork minimum", f"{precision} f{factor}", f"{own}:{rec8[0][1]},{rec8[0][2]}")
        _reset(eng)


# ---- 2. wide strips ------------------------------------------------------------------------------------------------------------------

WIDE_W = (32767, 32768, 32769, 65537, 100003)
WIDE_H = (1, 2, 5, 9)
F64_MAX_PX = 300_000


def _wide(eng, weights, factor, precision, h, w):
    import torch
    px = synth_u8(7 * w + h, 1, h, w)
    x = oracle.img_to_data(px)
    want32, want64 = _truth(weights, factor, f"wide{h}x{w}", x, f64=h * w <= F64_MAX_PX)
    for form in ("first", "pipe"):
        _force(eng, form)
        got32 = eng.upscale_f32(x)
        kind = _host_rec(eng)[0]
        _expect_final(eng, form, factor, precision, "f32", "f32", 3)
        _check(got32, want32, want64, TOL)
        got8 = eng.upscale_rgba8(px)
        _expect_final(eng, form, factor, precision, "u8", "u8", 3)
        np.testing.assert_array_equal(got8, _quantise(got32), err_msg=f"host u8 != quantised f32 {h}x{w} {form}")
        _check_u8(got8, want32)
        eng.set_experiment("fork", "0")
        d32 = eng.upscale_f32_dev(_dev(x))
        _expect_final(eng, form, factor, precision, "f32", "f32", 3)
        np.testing.assert_array_equal(d32.cpu().numpy(), got32, err_msg=f"device f32 != host {h}x{w} {form}")
        d8 = eng.upscale_rgba8_dev(_dev(px))
        _expect_final(eng, form, factor, precision, "u8", "u8", 3)
        np.testing.assert_array_equal(d8.cpu().numpy(), got8, err_msg=f"device u8 != host {h}x{w} {form}")
        if h == max(WIDE_H) and w == max(WIDE_W):
            d8a = eng.upscale_rgba8_dev(_dev(_with_alpha(px, h)))
            _expect_final(eng, form, factor, precision, "u8", "u8", 4)
            assert torch.equal(d8a, d8), (h, w, form)
        torch.cuda.synchronize()
        _cover("2 wide strips", f"{precision} f{factor}", f"{form} host:{kind}")
    _reset(eng)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_wide_strips_against_the_oracle(weights, engines, precision):
    eng = engines(3, precision)
    for w in WIDE_W:
        for h in WIDE_H:
            _wide(eng, weights, 3, precision, h, w)
    eng = engines(4, precision)
    for h in (1, 9):
        _wide(eng, weights, 4, precision, h, max(WIDE_W))


# ---- 3. many tiny images -------------------------------------------------------------------------------------------------------------

TINY = ((1, 1, 4096), (2, 3, 1500), (5, 7, 1000))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batches_of_tiny_images_against_the_oracle(weights, engines, precision):
    """Every image of the batch against the oracle, host and device, RGB and RGBA; the batch equal to one-image calls on a sample."""
    import torch
    eng = engines(3, precision)
    for (h, w, n) in TINY:
        px = synth_u8(n + h, n, h, w) if h > 1 else np.random.default_rng(n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        x = oracle.img_to_data(px)
        want32, want64 = _truth(weights, 3, f"tiny{n}x{h}x{w}", x)
        got32 = eng.upscale_f32(x)
        assert _host_rec(eng)[:2] == ("one", [n]), eng.get_experiment("plan")
        assert all((l["f"], l["prec"], l["img"], l["ch"]) == (3, precision, "f32", 3) for l in _finals(eng)), eng.get_experiment("plan")
        _check(got32, want32, want64, TOL)
        got8 = eng.upscale_rgba8(px)
        np.testing.assert_array_equal(got8, _quantise(got32))
        _check_u8(got8, want32)
        np.testing.assert_array_equal(eng.upscale_rgba8(_with_alpha(px, n)), got8)
        assert all(l["ch"] == 4 for l in _finals(eng))
        d32 = eng.upscale_f32_dev(_dev(x)).cpu().numpy()
        np.testing.assert_array_equal(d32, got32, err_msg=f"device batch != host batch {n}x{h}x{w}")
        d8 = eng.upscale_rgba8_dev(_dev(_with_alpha(px, n + 1))).cpu().numpy()
        assert all(l["ch"] == 4 for l in _finals(eng))
        np.testing.assert_array_equal(d8, got8, err_msg=f"device RGBA batch {n}x{h}x{w}")
        sample = sorted({0, 1, n // 2, n - 2, n - 1} | set(np.random.default_rng(h * w).integers(0, n, 4).tolist()))
        for i in sample:
            np.testing.assert_array_equal(eng.upscale_f32(x[i]), got32[i], err_msg=f"image {i} of {n}x{h}x{w}")
            np.testing.assert_array_equal(eng.upscale_rgba8_dev(_dev(px[i:i + 1])).cpu().numpy(), got8[i:i + 1])
        torch.cuda.synchronize()
        _cover("3 tiny batches", f"{precision} f3", f"{n}x{h}x{w} host:one")
    # a batch beyond one host chunk: per = 2^20 px / 4096 = 256 images of 64x64 -> chunks of 256 and 44
    n, h, w = 300, 64, 64
    px = synth_u8(300, n, h, w)
    x = oracle.img_to_data(px)
    want32, _ = _truth(weights, 3, "batch300", x, f64=False)
    got32 = eng.upscale_f32(x)
    assert _host_rec(eng)[:2] == ("batch", [256, 44]), eng.get_experiment("plan")
    _check(got32, want32, None, TOL)
    got8 = eng.upscale_rgba8(_with_alpha(px, 300))
    assert _host_rec(eng)[:2] == ("batch", [256, 44]), eng.get_experiment("plan")
    np.testing.assert_array_equal(got8, _quantise(got32))
    eng.set_pipeline(False)
    np.testing.assert_array_equal(eng.upscale_f32(x), got32)
    assert _host_rec(eng)[:2] == ("one", [n])
    _reset(eng)
    _cover("3 tiny batches", f"{precision} f3", "300x64x64 host:batch 256,44")


# ---- 4. planner corners --------------------------------------------------------------------------------------------------------------

def _mid_plan(h, w, precision, io):
    """plan_chunks' mid-size branch (sr_api.cpp), restated: None below mid_lo, "big" from 2^19 px, else the band rows."""
    split = precision == "split_f16"
    px = h * w
    mid_lo = (180000 if split else 200000) if io == "u8" else (140000 if split else 100000)
    if px < mid_lo:
        return None
    if px >= 1 << 19:
        return "big"
    if io == "f32" and px >= (300000 if split else 400000) and h >= 6 * SR_HALO:
        third = h // 3 // 8 * 8
        return [third, third, h - 2 * third]
    share = (0.6 if split else 0.7) if io == "u8" else (0.5 if split else 0.6)
    first = int(h * share) // 8 * 8
    return [first, h - first] if first >= 2 * SR_HALO and h - first >= 2 * SR_HALO else []


def _against_undivided(eng, px, io, what):
    """One host call (pipelined) of px, bit for bit against the undivided device call; returns the host plan it ran."""
    import torch
    eng.set_experiment("fork", "0")
    if io == "u8":
        want = eng.upscale_rgba8_dev(_dev(px[None]))[0].cpu().numpy()
    else:
        x = oracle.img_to_data(px)
        want = eng.upscale_f32_dev(_dev(x[None]))[0].cpu().numpy()
    assert eng.last_plan()["fork"] == [(False, 0, 0)]
    eng.set_experiment("fork", "")
    got = eng.upscale_rgba8(px) if io == "u8" else eng.upscale_f32(oracle.img_to_data(px))
    rec = _host_rec(eng)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(got, want, err_msg=f"{what}: host plan {rec} != undivided")
    return rec


@pytest.mark.parametrize("precision", PRECISIONS)
def test_host_plans_at_every_threshold(engines, precision):
    """Frames at each mid_lo threshold (100K / 140K / 180K / 200K px) and at 2^19 px, one row less and one more, u8 and f32 output."""
    eng = engines(3, precision)
    rng = np.random.default_rng(19)
    cases = [(1000, t) for t in (100, 140, 180, 200)] + [(1024, 512)]
    for (w, h0) in cases:
        for h in (h0 - 1, h0, h0 + 1):
            px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            for io in ("u8", "f32"):
                rec = _against_undivided(eng, px, io, f"{h}x{w} {io}")
                want = _mid_plan(h, w, precision, io)
                if not want:   # below mid_lo, or a mid-size frame too short for two bands of 2 SR_HALO rows
                    assert rec[0] == "one", (h, w, io, rec)
                elif want == "big":
                    assert rec[0] in ("inorder", "alternating") and len(rec[1]) >= 2 and sum(rec[1]) == h, (h, w, io, rec)
                else:
                    assert (rec[0], rec[1]) == ("inorder", want), (h, w, io, rec)
                _cover("4 thresholds", f"{precision} {io}", f"{h}x{w}:{rec[0]} {','.join(map(str, rec[1]))}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_band_plan_at_its_smallest(engines, precision):
    """f32 output, >= 400K px (split-half: 300K) and >= 6 SR_HALO rows: three bands in order, third = rows / 3 rounded down to 8 --
    bands of 8 rows, below the 2 SR_HALO floor the other branches keep.  A band of 8 own rows with 7 halo rows on each side is a
    valid band (the band entry points accept one own row): the bands must still give the undivided result."""
    eng = engines(3, precision)
    rng = np.random.default_rng(42)
    cases = [(42, 10000, [8, 8, 26]), (47, 10000, [8, 8, 31]),
             (42, 7200, [8, 8, 26] if precision == "split_f16" else _mid_plan(42, 7200, precision, "f32"))]
    for (h, w, want) in cases:
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rec = _against_undivided(eng, px, "f32", f"{h}x{w}")
        assert (rec[0], rec[1]) == ("inorder", want), (h, w, rec)
        assert want == _mid_plan(h, w, precision, "f32")
        _cover("4 three-band", precision, f"{h}x{w}:inorder {','.join(map(str, rec[1]))}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forced_band_plans_at_their_minimum(engines, precision):
    """"bands" at exactly 2 SR_HALO rows a band, "rows" with a band of one own row (in order and on alternating streams)."""
    eng = engines(3, precision)
    rng = np.random.default_rng(14)
    cases = [(28, 300, "bands", "2", ("alternating", [14, 14])), (42, 33, "bands", "3", ("alternating", [14, 14, 14])),
             (28, 300, "rows", "7,1,20", ("inorder", [7, 1, 20])), (28, 1, "rows", "7,1,20", ("inorder", [7, 1, 20])),
             (29, 300, "rows", "=14,1,14", ("alternating", [14, 1, 14])), (15, 300, "rows", "7,1,7", ("inorder", [7, 1, 7]))]
    for (h, w, key, val, want) in cases:
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        for io in ("u8", "f32"):
            _reset(eng)
            eng.set_experiment(key, val)
            rec = _against_undivided(eng, px, io, f"{h}x{w} {key}={val} {io}")
            assert (rec[0], rec[1]) == want, (h, w, key, val, io, rec)
            _cover("4 forced bands", f"{precision} {io}", f"{key}={val}:{rec[0]} {','.join(map(str, rec[1]))}")
    _reset(eng)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_band_entry_points_at_one_own_row(engines, precision):
    """sr_upscale_band_*_dev of ONE own row: halos 7 / 7 (h_ext = 15), and at the top and the bottom edge (halo 0 on that side) --
    the rows of the undivided call, W = 1 and W = 100 003, u8 RGB, u8 RGBA and f32."""
    import torch
    eng = engines(3, precision)
    f = 3
    for w in (1, 100003):
        px = synth_u8(w, 1, 15, w)[0]
        pxa = _with_alpha(px, w)
        x = oracle.img_to_data(px)
        d8, d8a, d32 = _dev(px), _dev(pxa), _dev(x)
        eng.set_experiment("fork", "0")
        want8, want32 = eng.upscale_rgba8_dev(d8[None])[0], eng.upscale_f32_dev(d32[None])[0]
        for (a, b, top, bot) in ((0, 15, 7, 7), (0, 8, 0, 7), (7, 15, 7, 0)):
            y = a + top
            for img, want in ((d8, want8), (d8a, want8)):
                got = eng.upscale_band_rgba8_dev(img[a:b].contiguous(), top, bot)
                assert _finals(eng)[0]["ch"] == img.shape[-1]
                assert eng.last_plan()["fork"] == [(False, 0, 0)]
                assert torch.equal(got, want[f * y:f * y + f]), (w, a, b, top, bot, img.shape[-1])
            got = eng.upscale_band_f32_dev(d32[a:b].contiguous(), top, bot)
            assert torch.equal(got, want32[f * y:f * y + f]), (w, a, b, top, bot)
            _cover("4 band entry", precision, f"W={w} row {y} halo {top}/{bot}")
        torch.cuda.synchronize()
    _reset(eng)


# ---- 5. buffer placement and streams -------------------------------------------------------------------------------------------------

def _carve(numel, dtype, offset, fill=0):
    """A contiguous view of `numel` elements starting `offset` elements into a larger device allocation."""
    import torch
    base = torch.full((numel + offset + 64,), fill, dtype=dtype, device="cuda")
    return base, base[offset:offset + numel]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_buffers_inside_larger_allocations_and_side_streams(engines, precision):
    """u8 RGB / RGBA inputs at byte offsets 0-3, f32 inputs and outputs 1-3 floats in, RGBA outputs at 4-byte offsets that are not
    16-byte aligned, whole-image, band and forked calls, on a side stream: the aligned, default-stream result bit for bit."""
    import torch
    eng = engines(3, precision)
    n, h, w = 2, 37, 75
    px = synth_u8(375, n, h, w)
    x = oracle.img_to_data(px)
    eng.set_experiment("fork", "0")
    want8 = eng.upscale_rgba8_dev(_dev(px))
    want32 = eng.upscale_f32_dev(_dev(x))
    torch.cuda.synchronize()
    for ch in (3, 4):
        src = px if ch == 3 else _with_alpha(px, ch)
        for off in range(4):
            base, view = _carve(src.size, torch.uint8, off)
            view.copy_(torch.from_numpy(src.reshape(-1)))
            img = view.view(src.shape)
            assert img.data_ptr() % 4 == off
            for oo in (4, 8, 12):
                obase, ov = _carve(want8.numel(), torch.uint8, oo, fill=7)
                out = ov.view(want8.shape)
                assert out.data_ptr() % 16 == oo
                eng.upscale_rgba8_dev(img, out=out)
                assert _finals(eng)[0]["ch"] == ch
                assert torch.equal(out, want8), (ch, off, oo)
                assert bool((obase[:oo] == 7).all()) and bool((obase[oo + out.numel():] == 7).all()), "wrote outside its view"
            _cover("5 placement", precision, f"u8 ch{ch} in+{off}B")
    for off in (1, 2, 3):
        base, view = _carve(x.size, torch.float32, off)
        view.copy_(torch.from_numpy(x.reshape(-1)))
        obase, ov = _carve(want32.numel(), torch.float32, off, fill=-1.0)
        out = ov.view(want32.shape)
        eng.upscale_f32_dev(view.view(x.shape), out=out)
        assert torch.equal(out, want32), off
        assert bool((obase[:off] == -1).all()) and bool((obase[off + out.numel():] == -1).all())
        _cover("5 placement", precision, f"f32 in/out+{off}f")
    # a band of the first image read from inside its batch at an odd byte offset, written inside a larger allocation
    _, view = _carve(px[0].size + 1, torch.uint8, 0)
    view[1:].copy_(torch.from_numpy(px[0].reshape(-1)))
    band = view[1:].view(h, w, 3)[2:29]                    # own rows 9..21, 7 halo rows each side
    assert band.is_contiguous() and band.data_ptr() % 2 == 1
    _, ov = _carve(13 * 3 * 3 * w * 4, torch.uint8, 4)
    eng.upscale_band_rgba8_dev(band, 7, 7, out=ov.view(39, 3 * w, 4))
    assert torch.equal(ov.view(39, 3 * w, 4), want8[0, 27:66])
    _cover("5 placement", precision, "band u8 in+1B out+4B")
    # side stream: whole, forked (own = 37 rows: cut "1" and 14) and band calls
    side = torch.cuda.Stream()
    d8, d32 = _dev(px[:1]), _dev(x[:1])
    for fork in ("0", "1", "14"):
        eng.set_experiment("fork", fork)
        with torch.cuda.stream(side):
            got8 = eng.upscale_rgba8_dev(d8, stream=side)
            rec8 = eng.last_plan()["fork"]
            got32 = eng.upscale_f32_dev(d32, stream=side)
        side.synchronize()
        assert rec8[0][0] == (fork != "0"), rec8
        assert torch.equal(got8, want8[:1]) and torch.equal(got32, want32[:1]), fork
        _cover("5 streams", precision, f"side stream fork {fork}: {rec8[0][1]},{rec8[0][2]}")
    _reset(eng)
    torch.cuda.synchronize()


def test_misaligned_outputs_are_refused(engines):
    """RGBA and f32 outputs (and f32 inputs) that are not 4-byte aligned: SR_E_INVALID before any launch, the output untouched --
    whole-image, band and sharded entry points, device and all-ranks forms."""
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    eng = engines(3, "f32")
    L = _lib.lib()
    h, w = 16, 20
    px = _dev(synth_u8(5, 1, h, w))
    x = _dev(oracle.img_to_data(synth_u8(5, 1, h, w)))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nout = 9 * h * w
    obase = torch.full((nout * 12 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    fbase = torch.full((x.numel() * 4 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    o = obase.data_ptr()
    fbase.view(-1)[1:1 + x.numel() * 4].copy_(x.view(-1).view(torch.uint8))
    f_mis = fbase.data_ptr() + 1
    ctx = eng._ctx
    V = C.c_void_p
    for off in (1, 2, 3):
        calls = {
            "rgba8_dev": lambda: L.sr_upscale_rgba8_dev(ctx, V(px.data_ptr()), 3, 1, h, w, V(o + off), s),
            "band_rgba8_dev": lambda: L.sr_upscale_band_rgba8_dev(ctx, V(px.data_ptr()), 3, h, w, 0, 0, V(o + off), s),
            "sharded_rgba8_dev": lambda: L.sr_upscale_sharded_rgba8_dev(ctx, V(px.data_ptr()), 3, h, w, V(o + off), s),
            "f32_dev out": lambda: L.sr_upscale_f32_dev(ctx, V(x.data_ptr()), 1, h, w, V(o + off), s),
            "band_f32_dev out": lambda: L.sr_upscale_band_f32_dev(ctx, V(x.data_ptr()), h, w, 0, 0, V(o + off), s),
            "sharded_f32_dev out": lambda: L.sr_upscale_sharded_f32_dev(ctx, V(x.data_ptr()), h, w, V(o + off), s),
            "f32_dev in": lambda: L.sr_upscale_f32_dev(ctx, V(f_mis), 1, h, w, V(o), s),
            "band_f32_dev in": lambda: L.sr_upscale_band_f32_dev(ctx, V(f_mis), h, w, 0, 0, V(o), s),
            "sharded_f32_dev in": lambda: L.sr_upscale_sharded_f32_dev(ctx, V(f_mis), h, w, V(o), s),
        }
        for name, call in calls.items():
            torch.cuda.synchronize()
            assert call() == _lib.SR_E_INVALID, (name, off)
            assert eng.last_plan()["launches"] == [], (name, eng.get_experiment("plan"))
            torch.cuda.synchronize()
            assert bool((obase == 0x5A).all()), f"{name} +{off}: output touched"
            _cover("5 refused", "f32", name)
    # the all-ranks forms, two contexts with local halo copies
    p = r.rsr.builtin("imagenet")
    sub = [r.Engine(p, device=0) for _ in range(2)]
    try:
        r.comm_init_all(sub, transport="local")
        ctxs = (V * 2)(*[e._ctx for e in sub])
        hb = (C.c_int * 2)(h // 2, h // 2)
        for off in (1, 2, 3):
            bands = (V * 2)(px.data_ptr(), px.data_ptr() + (h // 2) * w * 3)
            outs = (V * 2)(o, o + off + 4 * nout // 2)
            assert L.sr_upscale_sharded_rgba8_all(ctxs, 2, bands, 3, hb, w, outs) == _lib.SR_E_INVALID
            fb = (V * 2)(x.data_ptr(), f_mis)
            assert L.sr_upscale_sharded_f32_all(ctxs, 2, fb, hb, w, (V * 2)(o, o + 6 * nout)) == _lib.SR_E_INVALID
            fo = (V * 2)(o + off, o + 6 * nout)
            assert L.sr_upscale_sharded_f32_all(ctxs, 2, (V * 2)(x.data_ptr(), x.data_ptr() + (h // 2) * w * 12), hb, w, fo) \
                == _lib.SR_E_INVALID
            torch.cuda.synchronize()
            assert bool((obase == 0x5A).all()), f"sharded all +{off}: output touched"
        _cover("5 refused", "f32", "sharded_*_all")
    finally:
        for e in sub:
            e.close()
    # and 4-byte-aligned pointers into the same buffers are accepted
    assert L.sr_upscale_rgba8_dev(ctx, V(px.data_ptr()), 3, 1, h, w, V(o + 4), s) == _lib.SR_OK
    torch.cuda.synchronize()


# ---- coverage --------------------------------------------------------------------------------------------------------------------------

EXPECT = {
    "1 tall thin": lambda p, f: {"first/4", "pipe/4"} if (p, f) == ("split_f16", 4) else {"first/4", "first/8", "pipe/4", "pipe/8",
                                                                                          "pipe/8+4"},
}


def test_coverage_table():
    """Prints what every section above ran and asserted, from the plan records; holds the tall-thin matrix to its reachable cells."""
    lines = ["| section | column | asserted |", "|---|---|---|"]
    for section in sorted(COVERAGE):
        for col in sorted(COVERAGE[section]):
            lines.append(f"| {section} | {col} | " + "; ".join(sorted(COVERAGE[section][col])) + " |")
    print("\n" + "\n".join(lines))
    for col, cells in COVERAGE.get("1 tall thin", {}).items():
        p, f = col.split(" f")
        assert cells == EXPECT["1 tall thin"](p, int(f)), (col, cells)
