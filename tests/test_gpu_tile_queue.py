"""The stage kernels' tile queue held to the oracle at small shapes.

The persistent pipe form of the stage kernels (sr_kernels.hip conv_stage_pipe_kernel) asks its per-XCD tile queues only when a launch
has fewer workgroups than tiles -- on a 256-CU device from 512 tiles a launch, far above every shape the oracle comparisons run at.
sr_set_experiment("cus", "N") makes the planners plan for N compute units; with N of 1-5 the cases of tests/tile_queue_cases.py run the
queue, steals from queues no workgroup owns, the change of tile class inside a workgroup, 16 and more tiles through one workgroup and
the forked plans at shapes of a few thousand pixels (tests/test_tile_queue_cpu.py holds the table to what it claims to reach).

Every case, in this order: a decoy image of the same shape through the same engine under the same switches (the feature maps live on in
the workspace: a dropped tile would otherwise find the previous call's correct values in place), outputs filled with a sentinel; the
case; its plan record against the HIP-free planner's lines for that cus; output and all four nodes bit for bit against the same call
under "cus" = "" (behind a decoy too; nodes where both calls ran one undivided pass -- sr_read_feature refuses forked and banded calls);
three more calls, the same bytes each time; and, at shapes up to 61 x 97, output and nodes against the oracle at the bars of
tests/test_gpu_parity.py (TIGHT, scaled by the node's magnitude; the f64 truth by 2 max(|oracle f32 - truth|, 1e-6) + 1e-6; _check_u8)."""
import ctypes as C

import numpy as np
import pytest

import domain_cases as dc
import oracle
import param_families as pf
import plan_cases
import tile_queue_cases as tq
from conftest import synth_u8

pytestmark = pytest.mark.gpu

TOL = 1e-4          # north_star tolerance, pre-quantisation f32
TIGHT = 2e-5        # what exact-f32 MFMA actually achieves (rounding-order noise only): tests/test_gpu_parity.py
NODES = pf.NODES
MARGIN = {"f": 5, "l1": 3, "l2": 2, "l3": 1}  # rows a node is computed beyond a band's own (sr_plan.h kStageMargin)
SWITCHES = ("cus", "th", "pipe", "tail", "bw", "wino", "fork", "rows")
RESULTS = {}        # case name -> {"reached": set, "out": worst |gpu - oracle|, "truth": .., node: ..}: the coverage table


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


def _weights(factor):
    return pf.weights("imagenet", 3) if factor == 3 else pf.bundled_scale(factor, pf.seed_of(factor))


class Pool:
    """one engine per (factor, precision, purpose), the fork tuner off"""

    def __init__(self):
        self.engines = {}

    def get(self, factor, precision, purpose="cases"):
        import rusty_sr_amd as r
        key = (factor, precision, purpose)
        if key not in self.engines:
            e = r.Engine(_weights(factor), device=0, factor=factor, precision=precision)
            e.set_experiment("forktune", "0")
            self.engines[key] = e
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    return plan_cases.build_plan_check(tmp_path_factory.mktemp("plan_check"), sanitize=False)


@pytest.fixture(scope="module")
def planned(plan_check):
    return tq.plan_table(plan_check)


@pytest.fixture(scope="module")
def planned_plain(plan_check, pool):
    """the table planned for the device's own compute units: what "cus" = "" must run"""
    cus = pool.get(3, "f32").device_info()["compute_units"]
    status, err, out = plan_cases.run_plan_check(plan_check, [tq.planner_view(c) for c in tq.TABLE], cus)
    assert status == 0, err
    return {k: v[0] for k, v in out.items()}


def _plain(ctx):
    return [l for l in ctx if not l.startswith("#")]


# ---- images and the oracle ----
_IMAGES, _ORACLE = {}, {}


def _pixels(case, decoy):
    """(n, h, w, 3) u8 of the case's shape: one image per shape (both I/O kinds and every cus share its oracle run), another as the decoy"""
    key = (case["n"], case["h"], case["w"], decoy)
    if key not in _IMAGES:
        px = synth_u8(7000 + 1000 * decoy + 97 * case["h"] + case["w"] + case["n"], case["n"], case["h"], case["w"])
        assert px.any()
        px.flags.writeable = False
        _IMAGES[key] = px
    return _IMAGES[key]


def _input(case, decoy):
    """what the call is given: f32 data, or u8 pixels with a random alpha plane where the case reads RGBA"""
    px = _pixels(case, decoy)
    if case["io"] == "f32":
        return oracle.img_to_data(px)
    if case["ch"] == 4:
        a = np.random.default_rng(case["h"] + decoy).integers(0, 256, px.shape[:-1] + (1,), dtype=np.uint8)
        return np.ascontiguousarray(np.concatenate([px, a], axis=-1))
    return np.array(px)


def _truth(case):
    """(f32 output, f64 output, {node: f32 of image 0}) of the oracle on the case's image: one run per (factor, image), left unchanged"""
    key = (case["factor"], case["n"], case["h"], case["w"])
    if key not in _ORACLE:
        f, p = case["factor"], _weights(case["factor"])
        x = oracle.img_to_data(_pixels(case, False))
        o32, o64 = oracle.forward_factor(p, x, f), oracle.forward_factor(p, x, f, f64=True)
        taps = dc._taps(p, x[:1], f, False)
        for a in [o32, o64] + list(taps.values()):
            a.flags.writeable = False
        _ORACLE[key] = (o32, o64, taps)
    return _ORACLE[key]


# ---- one call ----
def _sentinel(out):
    out.fill(0xA5) if out.dtype == np.uint8 else out.fill(np.float32(np.nan))
    return out


def _call(eng, case, inp):
    """the case's call on `inp` into an output filled with a sentinel -> its bytes as a numpy array (n, f own rows, f w, 3 | 4)"""
    import torch
    f, n, h, w = case["factor"], case["n"], case["h"], case["w"]
    top, bot = case["halo"]
    u8 = case["io"] == "u8"
    shape = (n, f * (h - top - bot), f * w, 4 if u8 else 3)
    if case["call"] == "host":
        out = _sentinel(np.empty(shape, np.uint8 if u8 else np.float32))
        if u8:
            eng.upscale_rgba8(inp, out=out)
        else:  # (Engine.upscale_f32 allocates its result: the C entry point itself, into the filled array)
            from rusty_sr_amd import _lib
            fp = C.POINTER(C.c_float)
            _lib.check(eng._L.sr_upscale_f32(eng._ctx, inp.ctypes.data_as(fp), n, h, w, out.ctypes.data_as(fp)), eng._ctx)
        return out
    out = torch.full(shape, 0xA5 if u8 else float("nan"), dtype=torch.uint8 if u8 else torch.float32, device="cuda:0")
    d = torch.from_numpy(inp).cuda()
    if case["call"] == "band":
        (eng.upscale_band_rgba8_dev if u8 else eng.upscale_band_f32_dev)(d[0], top, bot, out=out[0])
    else:
        (eng.upscale_rgba8_dev if u8 else eng.upscale_f32_dev)(d, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _undivided(lines):
    """one pass over the whole call in the first workspace: sr_read_feature returns its nodes"""
    return lines[0] == "fork 0" or lines[0].startswith("host one")


def _rows(case, key):
    """the rows of node `key` a pass over the case's rows computes: a band's own and the margin its later stages read (the others keep
    what earlier calls left there)"""
    top, bot = case["halo"]
    h = case["h"]
    return slice(max(0, top - MARGIN[key]) if top else 0, min(h, h - bot + MARGIN[key]) if bot else h)


def _nodes(eng, case):
    return [eng.read_feature(k, case["h"], case["w"])[_rows(case, key)] for k, key in enumerate(NODES)]


def _set(eng, case, cus):
    for k in SWITCHES:
        eng.set_experiment(k, case["set"].get(k, ""))
    eng.set_experiment("cus", cus)


def _reset(eng):
    for k in SWITCHES:
        eng.set_experiment(k, "")


def _record(eng, case, want_lines):
    """the plan record of the last call against the planner's lines, and its launch words against the call's own arguments"""
    from rusty_sr_amd.engine import parse_plan
    text = eng.get_experiment("plan")
    assert plan_cases.canonical(text) == _plain(want_lines), (case["name"], text)
    for l in parse_plan(text)["launches"]:
        assert (l["prec"], l["f"], l["img"], l["out"], l["ch"]) == (case["precision"], case["factor"], case["io"], case["io"], case["ch"]), (case["name"], l)


@pytest.mark.parametrize("case", tq.TABLE, ids=[c["name"] for c in tq.TABLE])
def test_case(pool, planned, planned_plain, case):
    eng = pool.get(case["factor"], case["precision"])
    inp, decoy = _input(case, False), _input(case, True)
    assert inp.shape == decoy.shape and not np.array_equal(inp, decoy)
    lines = planned[case["id"]]
    reached = tq.reached(case, lines)
    assert set(case["reach"]) <= reached
    try:
        # 1. the decoy, 2. the case, 3. its plan record
        _set(eng, case, str(case["cus"]))
        decoy_out = _call(eng, case, decoy)
        got = _call(eng, case, inp)
        _record(eng, case, lines)
        assert not np.array_equal(got, decoy_out)
        nodes = _nodes(eng, case) if _undivided(_plain(lines)) else None
        # 5. three more times: the same bytes, whoever stole what
        for k in range(3):
            np.testing.assert_array_equal(_call(eng, case, inp), got, err_msg=f"{case['name']}: repeat {k} differs")
        if nodes is not None:
            for k, node in enumerate(_nodes(eng, case)):
                np.testing.assert_array_equal(node, nodes[k], err_msg=f"{case['name']}: node {NODES[k]} differs after the repeats")
        # 4. the same call planned for the device's own compute units, behind a decoy: the same bits
        _set(eng, case, "")
        _call(eng, case, decoy)
        ref = _call(eng, case, inp)
        _record(eng, case, planned_plain[case["id"]])
        np.testing.assert_array_equal(got, ref, err_msg=f"{case['name']}: output differs from the call under cus = \"\"")
        if nodes is not None and _undivided(_plain(planned_plain[case["id"]])):
            for k, node in enumerate(_nodes(eng, case)):
                np.testing.assert_array_equal(nodes[k], node, err_msg=f"{case['name']}: node {NODES[k]} differs from the call under cus = \"\"")
    finally:
        _reset(eng)
    res = RESULTS[case["name"]] = {"precision": case["precision"], "factor": case["factor"], "reached": reached}
    assert got.dtype == np.uint8 or np.isfinite(got).all(), case["name"]   # (no sentinel left)
    # 6. the oracle
    if not case["oracle"]:
        return
    f = case["factor"]
    top, bot = case["halo"]
    o32, o64, taps = _truth(case)
    own = slice(f * top, f * (case["h"] - bot))
    o32, o64 = o32[:, own], o64[:, own]
    if nodes is not None:
        for k, key in enumerate(NODES):
            want = taps[key][_rows(case, key)]
            res[key] = float(np.abs(nodes[k] - want).max())
            print(f"tile-queue {case['name']} {key}: |gpu - oracle| {res[key]:.3e}  max|oracle| {np.abs(want).max():.4g}")
            assert res[key] < TIGHT * max(1.0, np.abs(want).max()), (case["name"], key, res[key])
    if case["io"] == "u8":
        _check_u8(got, o32)
        res["u8"] = int(np.abs(got[..., :3].astype(int) - oracle.data_to_rgba8(o32)[..., :3].astype(int)).max())
        print(f"tile-queue {case['name']} out: u8 steps off the oracle {res['u8']}")
        return
    res["out"] = float(np.abs(got - o32).max())
    res["truth"] = float(np.abs(got.astype(np.float64) - o64).max())
    bound = 2 * max(float(np.abs(o32.astype(np.float64) - o64).max()), 1e-6) + 1e-6
    print(f"tile-queue {case['name']} out: |gpu - oracle| {res['out']:.3e}  |gpu - f64| {res['truth']:.3e}  bound {bound:.3e}")
    assert res["out"] < TIGHT, (case["name"], res["out"])
    assert res["truth"] < bound, (case["name"], res["truth"], bound)


# ---- 7. the split-half mode's domain flag from a tile that only a steal reaches ----
def _flagged(eng):
    """sr_check_domain once the device is idle: True for SR_E_DOMAIN, and the report is then gone"""
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    torch.cuda.synchronize()
    try:
        eng.check_domain()
    except r.SrError as e:
        assert e.status == _lib.SR_E_DOMAIN
        eng.check_domain()  # reported once
        return True
    return False


@pytest.mark.parametrize("node,b", [("l1", 31), ("l3", 0)])
@pytest.mark.parametrize("cus", [1, 3])
def test_domain_flag_from_a_stolen_tile(pool, plan_check, node, b, cus):
    """tests/domain_cases.py: ONE value of one node, at the last pixel of a 37 x 75 image, at 1.03 x 65504.  Planned for 1 / 3 compute
    units, tile order row-major ("bw" = "0"), that pixel lies in the launch's last tile, which the last XCD's queue holds alone -- a
    queue without an owner among 2 / 6 workgroups: the flag comes from a workgroup that stole the tile after its own queue ran dry.
    Status, sr_check_domain and the bytes -- the device call's and the host call's recomputed ones -- are what "cus" = "" gives; with
    the bright pixel taken out of the image the call is clean."""
    import torch
    c = dc.case(node, "last", b, "over", 3)
    H, W = dc.H, dc.W
    assert c.P == (H - 1, W - 1)
    shape = {"cus": cus, "precision": "split_f16", "h": H, "w": W, "factor": 3, "io": "f32", "call": "dev", "n": 1, "halo": [0, 0], "set": {},
             "pipeline": True, "profiling": False, "engines": 1, "id": 0}
    status, err, out = plan_cases.run_plan_check(plan_check, [shape], cus)
    assert status == 0, err
    lines = out[0][0]
    st = NODES.index(node)
    (nbig, nsmall, grid), = set(tq.queue_launches(shape, lines))   # every stage: the same 8-row tiles
    tx, ty = (W + 31) // 32, (H + 7) // 8
    assert nsmall == 0 and nbig == tx * ty and grid == 2 * cus < 8
    tile = nbig - 1
    assert tq.tile_coords(tile, tx, ty, 0) == (0, c.P[1] // 32, c.P[0] // 8)
    run = [x for x in range(8) if tq.run_of_xcd(x, nbig)[0] <= tile < sum(tq.run_of_xcd(x, nbig))]
    assert run == [7] and run[0] >= grid and tq.head_preset(grid)[7] == 0, (run, grid)   # no workgroup's own queue: a steal
    clean = np.array(c.x, copy=True)
    clean[0, c.P[0], c.P[1]] = clean[0, c.P[0], c.P[1] - 1]
    eng = pool.get(3, "split_f16", "domain")
    eng.set_params(c.params)
    try:
        seen = {}
        for setting in (str(cus), ""):
            eng.set_experiment("bw", "0")
            eng.set_experiment("cus", setting)
            eng.upscale_f32_dev(torch.from_numpy(clean).cuda())                  # (also the decoy)
            rec = plan_cases.canonical(eng.get_experiment("plan"))
            if setting:
                assert rec == _plain(lines), rec
            assert not _flagged(eng), (setting, "the image without the bright pixel is flagged")
            over = eng.upscale_f32_dev(torch.from_numpy(np.array(c.x)).cuda())
            flagged = _flagged(eng)
            feat = eng.read_feature(st, H, W)
            eng.upscale_f32(clean)
            host = eng.upscale_f32(np.array(c.x))                               # recomputed in f32 where the flag rose
            after = _flagged(eng)
            again = eng.upscale_f32_dev(torch.from_numpy(clean).cuda()).cpu().numpy()
            assert not _flagged(eng), (setting, "a stale flag")
            seen[setting] = (flagged, after, over.cpu().numpy(), feat, host, again)
        a, p = seen[str(cus)], seen[""]
        assert a[0] is True and p[0] is True, (a[0], p[0])
        assert a[1] == p[1]
        for k, what in ((2, "the device call's bytes"), (3, "the node"), (4, "the host call's recomputed bytes"), (5, "the clean call's bytes")):
            np.testing.assert_array_equal(a[k], p[k], err_msg=what)
    finally:
        _reset(eng)
        eng.set_params(_weights(3))


# ---- the switch itself ----
def test_the_switch_takes_one_to_the_devices_count_and_nothing_else(pool):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    eng = pool.get(3, "f32", "switch")
    info = eng.device_info()
    cus = info["compute_units"]
    x = oracle.img_to_data(synth_u8(5, 1, 24, 33))
    try:
        eng.set_experiment("cus", "1")
        want = eng.upscale_f32(x)
        one = eng.get_experiment("plan")
        assert "form=pipe ty8=2 ty4=2 grid=2" in one, one
        for bad in ("0", "-1", "+1", "1.5", " 2", "2 ", "abc", "0x2", str(cus + 1), "99999999999999999999"):
            with pytest.raises(r.SrError) as e:
                eng.set_experiment("cus", bad)
            assert e.value.status == _lib.SR_E_INVALID, bad
            np.testing.assert_array_equal(eng.upscale_f32(x), want)
            assert eng.get_experiment("plan") == one, bad        # a refused value leaves the switch as it was
        assert eng.device_info() == info                          # the device's own count stays what is reported
        eng.set_experiment("cus", "")
        np.testing.assert_array_equal(eng.upscale_f32(x), want)
        plain = eng.get_experiment("plan")
        assert plain != one
        eng.set_experiment("cus", str(cus))                       # the device's own count, spelt out: today's plan
        np.testing.assert_array_equal(eng.upscale_f32(x), want)
        assert eng.get_experiment("plan") == plain
        eng.set_experiment("cus", "2")
        eng.upscale_f32(x)
        two = eng.get_experiment("plan")
        assert two not in (one, plain)
        eng.set_experiment("cus", "002")                          # (decimal digits: leading zeros are none of its business)
        eng.upscale_f32(x)
        assert eng.get_experiment("plan") == two
    finally:
        _reset(eng)


def test_setting_the_switch_forgets_the_fork_tuners_measurements(pool):
    """40 x 70 planned for one compute unit is 7.5 rounds of tiles: inside the tuner's range, so with "forktune" on it starts measuring"""
    import torch
    eng = pool.get(3, "f32", "switch")
    x = torch.from_numpy(oracle.img_to_data(synth_u8(6, 1, 40, 70))).cuda()
    try:
        eng.set_experiment("forktune", "1")
        assert eng.get_experiment("forktune") == ""           # at the device's own count the shape is below the tuner's range
        eng.upscale_f32_dev(x)
        torch.cuda.synchronize()
        assert eng.get_experiment("forktune") == ""
        eng.set_experiment("cus", "1")
        want = eng.upscale_f32_dev(x)
        torch.cuda.synchronize()
        assert eng.get_experiment("forktune").startswith("40x70+0+0 f32 f32 measuring"), eng.get_experiment("forktune")
        eng.set_experiment("cus", "2")
        assert eng.get_experiment("forktune") == ""
        assert torch.equal(eng.upscale_f32_dev(x), want)
        torch.cuda.synchronize()
    finally:
        eng.set_experiment("forktune", "0")
        _reset(eng)


# ---- 8. the coverage table ----
def test_coverage_table():
    """case x properties reached x worst error; with the whole table run, every property is reached in both precisions"""
    print("\ntile-queue coverage: case | reached | worst |gpu - oracle|: out, |gpu - f64|, f, l1, l2, l3 (u8 calls: steps off)")
    for name, r in RESULTS.items():
        errs = "  ".join(f"{k} {r[k]:.2e}" if k != "u8" else f"u8 {r[k]}" for k in ("out", "truth", "u8") + NODES if k in r)
        print(f"  {name:64s} | {' '.join(p for p in tq.PROPERTIES if p in r['reached']):55s} | {errs or '(plan, bit identity and repeatability only)'}")
    print("tile-queue errors: worst per precision, factor and node over the cases held to the oracle")
    for prec in tq.PRECISIONS:
        for factor in (2, 3, 4):
            rows = [r for r in RESULTS.values() if (r["precision"], r["factor"]) == (prec, factor)]
            worst = {k: max(r[k] for r in rows if k in r) for k in ("out", "truth", "u8") + NODES if any(k in r for r in rows)}
            print(f"  {prec:9s} factor {factor}: " + "  ".join(f"{k} {v:.3e}" if k != "u8" else f"u8 {v}" for k, v in worst.items()))
    if len(RESULTS) == len(tq.TABLE):
        for prec in tq.PRECISIONS:
            got = set().union(*(r["reached"] for r in RESULTS.values() if r["precision"] == prec))
            assert got == set(tq.PROPERTIES), (prec, sorted(set(tq.PROPERTIES) - got))
