"""Every form of the final stage, at every factor, in both arithmetic modes -- and the call paths around it at factors 2 and 4 and with
RGBA input -- each with the plan record (sr_get_experiment "plan", Engine.last_plan) asserting that the intended kernel ran.

The library chooses tile classes, kernel forms and band plans itself, and its thresholds move; a test that meant to run one kernel can
end up running another without noticing.  Here every call is followed by an assertion on what it ran.

Cells: precision {f32, split_f16} x factor {2, 3, 4} x final-stage form {first form / 4-row tiles, first form / 8-row tiles, pipe form /
4-row tiles, pipe form / 8-row tiles (the exact mode: the 4x4x1 "quad" MFMA path), pipe form / 8-row tiles ended by 4-row tiles}.
The split-half mode's final stage at factor 4 exists with 4-row tiles only (sr_kernels.hip kBigTiles): a request for 8-row tiles there
must still record 4-row tiles.  Each cell's f32 output is held against the C oracle (f32) and against exact arithmetic (its f64 leg);
its u8 output must be the quantised f32 output bit for bit, and RGBA input (a random alpha plane) must give the RGB result."""
import numpy as np
import pytest

import oracle
from conftest import synth_u8
from param_families import bundled_scale as _synthetic_params   # (the one generator of bundled-scale weights)

pytestmark = pytest.mark.gpu

TOL = 1e-4          # north_star tolerance, pre-quantisation f32
TIGHT = 2e-5        # what exact-f32 MFMA actually achieves (rounding-order noise only)

PRECISIONS = ("f32", "split_f16")
FORMS = {  # the switches that force each cell (sr_set_experiment); the mixed cell is reached on an image of >= 2 rounds of 8-row tiles
    "first/4": {"pipe": "none", "th": "4"},
    "first/8": {"pipe": "none", "th": "8"},
    "pipe/4": {"pipe": "all", "th": "4"},
    "pipe/8": {"pipe": "all", "th": "8"},
    "pipe/8+4": {"tail": "1"},
}
SWITCHES = ("pipe", "th", "tail", "bw", "fork", "forktune")


def _check_u8(got, v_ref):
    want = oracle.data_to_rgba8(v_ref)
    assert got.shape == want.shape
    assert (got[..., 3] == 255).all()
    d = got[..., :3].astype(int) - want[..., :3].astype(int)
    assert np.abs(d).max() <= 1
    if (d != 0).any():
        frac = 255.0 * v_ref.astype(np.float64) + 0.5
        edge = np.abs(frac - np.round(frac))
        assert edge[d != 0].max() < 255 * TOL, "u8 mismatch away from a rounding knife-edge"
        assert (d != 0).mean() < 1e-3


def _quantise(v):
    """data_to_img as the kernels compute it: clamp(floor(255 v + 0.5), 0, 255) in f32 arithmetic, alpha 255."""
    v = np.asarray(v, dtype=np.float32)
    q = np.clip(np.floor(v * np.float32(255.0) + np.float32(0.5)), 0, 255).astype(np.uint8)
    return np.concatenate([q, np.full(v.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def _with_alpha(px, seed):
    """RGBA: a random alpha plane (a constant one would hide a kernel that reads it)."""
    a = np.random.default_rng(seed).integers(0, 256, px.shape[:-1] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([px, a], axis=-1))


@pytest.fixture(scope="module")
def weights(params):
    return {2: _synthetic_params(2, 102), 3: params["imagenet"], 4: _synthetic_params(4, 104)}


_ORACLE = {}


def _truth(weights, factor, name, x):
    """One oracle run (f32 and f64) per (factor, image), shared by both precisions and every form."""
    key = (factor, name)
    if key not in _ORACLE:
        _ORACLE[key] = (oracle.forward_factor(weights[factor], x, factor), oracle.forward_factor(weights[factor], x, factor, f64=True))
    return _ORACLE[key]


def _reset(eng):
    for k in SWITCHES:
        eng.set_experiment(k, "")
    eng.set_pipeline(True)


def _final(eng, n_final=1):
    """The final-stage launch(es) of the last call, from the plan record."""
    fin = [l for l in eng.last_plan()["launches"] if l["st"] == 4]
    assert sum(l["count"] for l in fin) == n_final, eng.get_experiment("plan")
    return fin[0]


def _cell_of(l):
    return f"{l['form']}/" + ("8+4" if l["ty8"] and l["ty4"] else "8" if l["ty8"] else "4")


def _expect_cell(eng, form, factor, precision, img, out, ch):
    l = _final(eng)
    assert (l["f"], l["prec"], l["img"], l["out"], l["ch"]) == (factor, precision, img, out, ch), l
    want = form
    if precision == "split_f16" and factor == 4:
        want = form.split("/")[0] + "/4"   # kBigTiles: the 4-row body only, whatever was requested
    assert _cell_of(l) == want, (form, eng.get_experiment("plan"))
    return _cell_of(l)


COVERAGE = {}  # (precision, factor) -> final-stage cells seen (for the table printed by test_coverage_table)


def _check_f32(got, want32, want64, tol):
    assert got.shape == want32.shape
    assert np.abs(got - want32).max() < tol
    # against exact arithmetic the GPU is as close as the CPU f32 path is
    bound = 2 * np.abs(want32.astype(np.float64) - want64).max() + 1e-7
    assert np.abs(got.astype(np.float64) - want64).max() <= bound


def _run_cell(eng, form, factor, precision, px, x, want32, want64, tol, seed):
    """One cell on one image: f32 against the oracle and the f64 truth, u8 = quantised f32 bit for bit, RGBA = RGB."""
    got32 = eng.upscale_f32(x)
    COVERAGE.setdefault((precision, factor), set()).add(_expect_cell(eng, form, factor, precision, "f32", "f32", 3))
    _check_f32(got32, want32, want64, tol)
    got8 = eng.upscale_rgba8(px)
    _expect_cell(eng, form, factor, precision, "u8", "u8", 3)
    np.testing.assert_array_equal(got8, _quantise(got32), err_msg=f"u8 != quantised f32 ({form})")
    _check_u8(got8, want32)
    got8a = eng.upscale_rgba8(_with_alpha(px, seed))
    _expect_cell(eng, form, factor, precision, "u8", "u8", 4)
    np.testing.assert_array_equal(got8a, got8, err_msg=f"RGBA != RGB ({form})")
    return got32, got8


@pytest.mark.parametrize("factor", [2, 3, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_final_stage_cells_against_the_oracle(weights, factor, precision):
    import rusty_sr_amd as r
    eng = r.Engine(weights[factor], device=0, factor=factor, precision=precision)
    rng = np.random.default_rng(factor)
    small = {
        # a batch of two with a ragged width (75 = 2 x 32 + 11) and height (37 = 4 x 8 + 5): partial tiles on both sides
        "synth": (synth_u8(200 + factor, 2, 37, 75), TIGHT),
        # white noise drives pre-activations to +-70: the f64 bound is the yardstick, the f32 one the north star
        "noise": (rng.integers(0, 256, (1, 45, 96, 3), dtype=np.uint8), TOL),
    }
    try:
        eng.set_pipeline(False)   # one chunk per host call: the forced switches apply to the one launch of each stage
        for name, (px, tol) in small.items():
            x = oracle.img_to_data(px)
            want32, want64 = _truth(weights, factor, name, x)
            for form in ("first/4", "first/8", "pipe/4", "pipe/8"):
                _reset(eng)
                eng.set_pipeline(False)
                for k, v in FORMS[form].items():
                    eng.set_experiment(k, v)
                _run_cell(eng, form, factor, precision, px, x, want32, want64, tol, seed=len(name))
        # the mixed cell: 8-row tiles ended by 4-row tiles needs >= 2 rounds of 8-row tiles (2 x 512 on 256 CUs): 33 x 33 = 1089 tiles
        px = synth_u8(300 + factor, 1, 264, 1056)
        x = oracle.img_to_data(px)
        want32, want64 = _truth(weights, factor, "big", x)
        _reset(eng)
        eng.set_pipeline(False)
        eng.set_experiment("tail", FORMS["pipe/8+4"]["tail"])
        mixed32, mixed8 = _run_cell(eng, "pipe/8+4", factor, precision, px, x, want32, want64, TIGHT, seed=3)
        stages = [l for l in eng.last_plan()["launches"] if 1 <= l["st"] <= 3]
        assert all(l["form"] == "pipe" and l["ty8"] and l["ty4"] for l in stages), eng.get_experiment("plan")
        # ... and bit for bit what the 8-row pipe form computes on the same image (the forms share step order and weight chunks)
        _reset(eng)
        eng.set_pipeline(False)
        eng.set_experiment("pipe", "all")
        eng.set_experiment("th", "8")
        np.testing.assert_array_equal(eng.upscale_f32(x), mixed32)
        np.testing.assert_array_equal(eng.upscale_rgba8(px), mixed8)
        # the natural case: a lone image of >= 3 rounds of tiles whose height leaves 3 rows (403 = 50 x 8 + 3), through a device entry
        # point undivided -- the exact mode ends its final stage with ONE row of 4-row tiles, the split-half mode keeps 8-row tiles
        _natural(eng, weights, factor, precision)
    finally:
        eng.close()


def _natural(eng, weights, factor, precision):
    import torch
    px = synth_u8(400 + factor, 1, 403, 1100)
    x = oracle.img_to_data(px)
    want32, want64 = _truth(weights, factor, "natural", x)
    _reset(eng)
    eng.set_experiment("fork", "0")
    got32 = eng.upscale_f32_dev(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    rec = eng.last_plan()
    assert rec["fork"] == [(False, 0, 0)], eng.get_experiment("plan")
    cell = _cell_of(_final(eng))
    want = "pipe/8+4" if precision == "f32" else ("pipe/4" if factor == 4 else "pipe/8")
    assert cell == want, eng.get_experiment("plan")
    if precision == "f32":
        l = _final(eng)
        assert (l["ty8"], l["ty4"]) == (50, 1), l
    COVERAGE.setdefault((precision, factor), set()).add(cell)
    got32 = got32.cpu().numpy()
    _check_f32(got32, want32, want64, TIGHT)
    got8 = eng.upscale_rgba8_dev(torch.from_numpy(px).cuda()).cpu().numpy()
    assert _cell_of(_final(eng)) == want
    np.testing.assert_array_equal(got8, _quantise(got32))
    _check_u8(got8, want32)
    got8a = eng.upscale_rgba8_dev(torch.from_numpy(_with_alpha(px, 9)).cuda()).cpu().numpy()
    l = _final(eng)
    assert _cell_of(l) == want and l["ch"] == 4
    np.testing.assert_array_equal(got8a, got8)
    _reset(eng)


def test_coverage_table():
    """Prints the cell x factor x precision table of what the matrix above ran (from the plan records) and holds every (precision,
    factor) that ran to its reachable cells: all five, except the split-half mode at factor 4 (4-row final stage only)."""
    cells = ("first/4", "first/8", "pipe/4", "pipe/8", "pipe/8+4")
    ran = [(p, f) for p in PRECISIONS for f in (2, 3, 4) if (p, f) in COVERAGE]   # (all six in a run of the whole module)
    lines = ["| final stage | " + " | ".join(f"{p} f{f}" for p, f in ran) + " |"]
    for c in cells:
        lines.append(f"| {c} | " + " | ".join("x" if c in COVERAGE[k] else "-" for k in ran) + " |")
    print("\n" + "\n".join(lines))
    for p, f in ran:
        want = set(cells) if not (p == "split_f16" and f == 4) else {"first/4", "pipe/4"}
        assert COVERAGE[(p, f)] == want, (p, f, COVERAGE[(p, f)])


# ---- the call paths at factors 2 and 4, and with RGBA input -------------------------------------------------------------------------
# Everything below is bit for bit against the same context's undivided pass (set_pipeline(False) for host calls, "fork" = "0" for
# device calls), which the matrix above has tied to the oracle.

def _host_kind(host, io):
    kind, sizes, _ = host
    if kind in ("one", "batch"):
        return kind
    if kind == "inorder":
        if len(sizes) == 2:
            return f"inorder-2 {io}"
        if all(a > b for a, b in zip(sizes, sizes[1:])):
            return "geometric"
        if len(sizes) == 3 and sizes[0] == sizes[1]:
            return "inorder-3"
        return "equal-inorder"
    return "alternating-equal" if max(sizes) - min(sizes) <= 1 else "big+tail"


HOST_KINDS = {}  # (precision, factor) -> kinds seen


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_host_plans_are_bit_identical(weights, factor, precision):
    """Every chunk plan the host-pointer selector (plan_chunks) can produce at this factor -- one chunk, batch chunks, mid-size bands
    in order (u8 and f32 output), three in order, geometric bands, equal bands in order, equal bands on alternating streams, two big
    bands and a tail -- RGB and RGBA, pageable and page-locked destinations: the bytes of the undivided pass."""
    import rusty_sr_amd as r
    from rusty_sr_amd.engine import host_alloc
    eng = r.Engine(weights[factor], device=0, factor=factor, precision=precision)
    cases = [  # n, h, w, io, channels, page-locked destination
        (1, 300, 515, "u8", 3, False), (1, 300, 515, "f32", 3, False),
        (1, 480, 640, "u8", 4, True), (1, 480, 640, "f32", 3, False),
        (1, 600, 800, "u8", 3, False), (1, 600, 800, "f32", 3, False),
        (1, 600, 1000, "u8", 4, False), (1, 600, 1000, "f32", 3, False),
        (1, 1080, 1920, "u8", 4, True), (1, 1080, 1920, "f32", 3, False),
        (3, 600, 600, "u8", 4, False), (9, 300, 300, "u8", 3, False),
    ]
    if factor == 2:   # geometric u8 bands need >= 3 of >= 300K px (f = 4 never takes that plan: its kernels are shorter than the download)
        cases.append((1, 2160, 1920, "u8", 3, True))
    seen = HOST_KINDS.setdefault((precision, factor), set())
    try:
        for (n, h, w, io, ch, pinned) in cases:
            px = synth_u8(h + w + n, n, h, w)
            f = factor
            if io == "u8":
                src = _with_alpha(px, h) if ch == 4 else px
                eng.set_pipeline(False)
                want = eng.upscale_rgba8(px)
                assert [k for k, _, _ in eng.last_plan()["host"]] == ["one"]
                eng.set_pipeline(True)
                if pinned:
                    buf = host_alloc((n, f * h, f * w, 4))
                    got = eng.upscale_rgba8(src, out=buf.array).copy()
                    rec = eng.last_plan()
                    buf.close()
                else:
                    got = eng.upscale_rgba8(src)
                    rec = eng.last_plan()
            else:
                x = oracle.img_to_data(px)
                eng.set_pipeline(False)
                want = eng.upscale_f32(x)
                eng.set_pipeline(True)
                got = eng.upscale_f32(x)
                rec = eng.last_plan()
            assert len(rec["host"]) == 1, rec
            kind = _host_kind(rec["host"][0], io)
            seen.add(kind)
            print(f"{precision} f{factor} {n}x{h}x{w} {io} ch{ch}: {kind} {rec['host'][0][0]} {rec['host'][0][1]}")
            finals = [l for l in rec["launches"] if l["st"] == 4]
            assert all(l["ch"] == (ch if io == "u8" else 3) and l["f"] == factor for l in finals)
            np.testing.assert_array_equal(got, want, err_msg=f"{(n, h, w, io, ch)}: {kind}")
    finally:
        _reset(eng)
        eng.close()
    expect = {"one", "batch", "inorder-2 u8", "inorder-2 f32", "inorder-3", "alternating-equal", "equal-inorder"}
    if factor == 2:
        expect |= {"geometric", "big+tail"}
    assert seen == expect, (precision, factor, seen)


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forked_device_calls_are_bit_identical(weights, factor, precision):
    """sr_upscale_*_dev as two row bands on two streams (sr_run_stack_auto): cut "1" (the planned cut), 14 rows, an odd cut and the
    automatic rule; whole images and bands with 7 / 9 + 8 halo rows; u8 RGB, u8 RGBA and f32; on a side stream."""
    import torch
    import rusty_sr_amd as r
    eng = r.Engine(weights[factor], device=0, factor=factor, precision=precision)
    rng = np.random.default_rng(500 + factor)
    side = torch.cuda.Stream()
    try:
        eng.set_experiment("forktune", "0")   # the automatic case below is the rule's, not the tuner's measurement
        for (h, w, top, bot) in ((131, 257, 0, 0), (300, 515, 0, 0), (90, 333, 7, 7), (83, 640, 9, 8), (600, 900, 0, 0)):
            px3 = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
            px4 = torch.from_numpy(_with_alpha(px3.cpu().numpy(), h)).cuda()
            x = torch.from_numpy(oracle.img_to_data(px3.cpu().numpy())).cuda()
            band = top or bot
            def run8(px, stream=None):
                return eng.upscale_band_rgba8_dev(px, top, bot, stream=stream) if band else eng.upscale_rgba8_dev(px[None], stream=stream)[0]
            def run32(stream=None):
                return eng.upscale_band_f32_dev(x, top, bot, stream=stream) if band else eng.upscale_f32_dev(x[None], stream=stream)[0]
            eng.set_experiment("fork", "0")
            want8, want32 = run8(px3), run32()
            torch.cuda.synchronize()
            assert eng.last_plan()["fork"] == [(False, 0, 0)]
            own = h - top - bot
            cuts = ["1"] + [str(c) for c in (14, 2 * (own // 4) + 1) if 14 <= c <= own - 14]
            if (h, w) == (600, 900):
                cuts = ["1", ""]   # 4.2 rounds of tiles: the automatic rule forks in the exact mode, not in the split-half mode
            for cut in cuts:
                eng.set_experiment("fork", cut)
                with torch.cuda.stream(side):
                    got8 = run8(px3, side)
                    fork8 = eng.last_plan()["fork"]
                    got8a = run8(px4, side)
                    fork8a = eng.last_plan()["fork"]
                    got32 = run32(side)
                    fork32 = eng.last_plan()["fork"]
                    same = torch.equal(got8, want8), torch.equal(got8a, want8), torch.equal(got32, want32)
                assert all(same), (h, w, top, bot, cut, same)
                forked = cut != "" or precision == "f32"
                for rec in (fork8, fork8a, fork32):
                    assert len(rec) == 1 and rec[0][0] == forked, (cut, rec)
                    if forked:
                        assert rec[0][1] + rec[0][2] == own
                    if cut not in ("", "1"):
                        assert rec[0][1] == int(cut)
    finally:
        _reset(eng)
        eng.close()


@pytest.mark.parametrize("factor", [2, 4])
def test_multi_context_and_sharded_calls_are_bit_identical(weights, factor):
    """sr_upscale_*_multi over 1-3 contexts, sr_upscale_*_batch_multi with 2 and 3 contexts and a ragged batch, and
    sr_comm_init_local + sr_upscale_sharded_*_all with 2 and 3 ranks (halo "input" and "layers", uneven bands) -- u8 RGB, RGBA, f32."""
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd.shard import split_rows
    engs = [r.Engine(weights[factor], device=0, factor=factor) for _ in range(3)]
    try:
        e0 = engs[0]
        for (h, w) in ((37, 50), (600, 900)):
            px = synth_u8(h + factor, 1, h, w)[0]
            x = oracle.img_to_data(px)
            e0.set_pipeline(False)
            want8, want32 = e0.upscale_rgba8(px), e0.upscale_f32(x)
            e0.set_pipeline(True)
            for k in (1, 2, 3):
                np.testing.assert_array_equal(r.upscale_multi(engs[:k], x), want32, err_msg=f"f32 {h}x{w} on {k}")
                np.testing.assert_array_equal(r.upscale_multi(engs[:k], _with_alpha(px, k)), want8, err_msg=f"RGBA {h}x{w} on {k}")
                if k > 1 and h > 100:
                    shares = [e.last_plan()["host"] for e in engs[:k]]
                    assert all(len(s) == 1 and s[0][2] is not None for s in shares), shares
                    assert sum(s[0][2][1] - s[0][2][0] for s in shares) == h
                    assert all(l["ch"] == 4 for e in engs[:k] for l in e.last_plan()["launches"])
        pxb = synth_u8(77 + factor, 5, 45, 70)
        xb = oracle.img_to_data(pxb)
        e0.set_pipeline(False)
        want8b, want32b = e0.upscale_rgba8(pxb), e0.upscale_f32(xb)
        e0.set_pipeline(True)
        for k in (2, 3):
            np.testing.assert_array_equal(r.upscale_batch_multi(engs[:k], _with_alpha(pxb, k)), want8b, err_msg=f"batch RGBA on {k}")
            np.testing.assert_array_equal(r.upscale_batch_multi(engs[:k], xb), want32b, err_msg=f"batch f32 on {k}")
            assert [e.last_plan()["host"][0][1] for e in engs[:k]] == [[len(range(j, 5, k))] for j in range(k)]
        # sharded: contexts of one device, halos by peer copy
        H, W = 37 * 3 + 5, 300
        px = synth_u8(31 + factor, 1, H, W)[0]
        e0.set_pipeline(False)
        want8, want32 = e0.upscale_rgba8(px), e0.upscale_f32(oracle.img_to_data(px))
        e0.set_pipeline(True)
        x = oracle.img_to_data(px)
        for n in (2, 3):
            sub = [r.Engine(weights[factor], device=0, factor=factor) for _ in range(n)]
            try:
                r.comm_init_all(sub, transport="local")
                uneven = [7] * (n - 1) + [H - 7 * (n - 1)]
                edges = np.cumsum([0] + uneven)
                for halo in ("input", "layers"):
                    for e in sub:
                        e.set_experiment("halo", halo)
                    for cuts in (split_rows(H, n), list(zip(edges[:-1], edges[1:]))):
                        outs = r.upscale_sharded_all(sub, [torch.from_numpy(_with_alpha(px[a:b], a)).cuda() for a, b in cuts])
                        np.testing.assert_array_equal(np.concatenate([o.cpu().numpy() for o in outs]), want8, err_msg=f"RGBA {n} {halo}")
                        assert all(l["ch"] == 4 and l["f"] == factor for e in sub for l in e.last_plan()["launches"])
                        outs = r.upscale_sharded_all(sub, [torch.from_numpy(x[a:b]).cuda() for a, b in cuts])
                        np.testing.assert_array_equal(np.concatenate([o.cpu().numpy() for o in outs]), want32, err_msg=f"f32 {n} {halo}")
            finally:
                for e in sub:
                    e.close()
    finally:
        for e in engs:
            e.close()


def test_fork_tuner_and_reserve_with_rgba_at_factor_4(weights):
    """A mid-size factor-4 RGBA shape (1.5 rounds of tiles: the fork tuner measures it): ten fenced calls, undivided and forked while it
    measures, never change a byte; sr_reserve_rgba8(.., 4, ..) and then the call gives what a context that never reserved gives."""
    import torch
    import rusty_sr_amd as r
    h, w = 448, 448
    px = _with_alpha(synth_u8(448, 1, h, w), 4)
    eng = r.Engine(weights[4], device=0, factor=4)
    try:
        d = torch.from_numpy(px).cuda()
        eng.set_experiment("fork", "0")
        want = eng.upscale_rgba8_dev(d)
        torch.cuda.synchronize()
        eng.set_experiment("fork", "")
        eng.set_experiment("forktune", "1")
        forks = set()
        for k in range(10):
            assert torch.equal(eng.upscale_rgba8_dev(d), want), k
            forks.add(eng.last_plan()["fork"][0][0])
            torch.cuda.synchronize()
        assert forks == {False, True}   # both plans were measured
        lines = [l.split() for l in eng.get_experiment("forktune").splitlines()]
        assert any(l[0] == f"{h}x{w}+0+0" and l[3] in ("undivided", "forked") for l in lines), lines
        eng.set_pipeline(False)
        plain = eng.upscale_rgba8(px)
        np.testing.assert_array_equal(plain, want.cpu().numpy())
    finally:
        _reset(eng)
        eng.close()
    eng = r.Engine(weights[4], device=0, factor=4)
    try:
        eng.reserve(1, h, w, io="rgba8", channels=4)
        rec = eng.last_plan()
        assert rec["host"] and all(l["ch"] == 4 for l in rec["launches"]), rec
        np.testing.assert_array_equal(eng.upscale_rgba8(px), plain)
    finally:
        eng.close()
