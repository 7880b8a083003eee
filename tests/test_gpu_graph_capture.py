"""Every *_dev entry point held to its stream-capture contract (include/srhip.h "Stream capture"): one call captured and replayed on
changing inputs (tests/graph_capture.py has the helper and the table), graphs of two geometries that share one allocation interleaved with
eager and host-pointer calls, one graph of a train of calls, a cold call inside a capture, the domain flag and the fork tuner under replay.
Bit for bit throughout: the reference is the same call made eagerly, which the other GPU tests hold to the oracle.

No graph is replayed after anything that could grow or free what it points to (a larger shape, sr_set_params, sr_set_precision,
sr_destroy): every shape a test uses has run eagerly on the context before its first capture, a context is grown only after its graphs
are destroyed, and point 3 of the contract is documented, not exercised.

Run with -s to see the coverage table at the end."""
import gc as pygc
import time

import numpy as np
import pytest

import graph_capture as gc
import stream_order as so

pytestmark = pytest.mark.gpu

RESULTS = {}    # row id -> the legs replayed() ran; the coverage table is printed from it
EXTRA = {}      # test -> one line for the table
T0 = time.perf_counter()
A, B = (37, 75), (30, 90)   # LR shapes of three column tiles each, hence one pitch: each has interior where the other has border
COLD = (64, 160)            # larger than anything a context of these tests is warm for


@pytest.fixture(scope="module")
def weights(params):
    from param_families import bundled_scale
    return {2: bundled_scale(2, 102), 3: params["imagenet"], 4: bundled_scale(4, 104)}


@pytest.fixture(scope="module")
def stream():
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.zeros(16, device="cuda").add_(1)
    torch.cuda.synchronize()
    return s


@pytest.fixture
def make(weights):
    """Fresh engines for one test, closed after it (and after its graphs: a test deletes them itself)."""
    import rusty_sr_amd as r
    made = []

    def fresh(factor=3, precision="f32", **kw):
        e = r.Engine(weights[factor] if kw.get("graph", "sr_net") == "sr_net" else (), device=0, factor=factor, precision=precision, **kw)
        made.append(e)
        return e
    yield fresh
    import torch
    pygc.collect()
    torch.cuda.synchronize()
    for e in made:
        e.close()


def _status(fn):
    """the status a call raises, SR_OK where it raises nothing"""
    from rusty_sr_amd import _lib
    try:
        fn()
    except _lib.SrError as e:
        return e.status
    return _lib.SR_OK


# ---- (a) every row ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", gc.ROWS, ids=[r["id"] for r in gc.ROWS])
def test_replayed(make, weights, stream, row):
    """One row of the table: the call captured once and replayed on changing inputs (tests/graph_capture.py)."""
    eng = make(row["factor"], row["precision"])
    eng.set_experiment("fork", row["fork"] or "")
    case = getattr(so.Builders(eng, weights[row["factor"]]), row["build"])()

    def check_after():
        if row["fork"]:   # the captured call ran as two bands: the graph has the second stream's branch
            assert eng.last_plan()["fork"] and eng.last_plan()["fork"][0][0], eng.get_experiment("plan")
        if row["precision"] == "split_f16":
            eng.check_domain()
    RESULTS[row["id"]] = gc.replayed(case, stream, check_after, name=row["id"])


# ---- (b) two geometries in one allocation ------------------------------------------------------------------------------------------------------
INTERLEAVED = ["plain_u8", "plain_f32", "band_u8", "ensemble_u8", "border_u8", "sized", "upscale_yuv", "upscale_u16", "valid", "backprop"]


def _interleaved_params():
    out = []
    for build in INTERLEAVED:
        for precision in (("f32", "split_f16") if build in so.NETWORK.values() else ("f32",)):
            out.append((build, precision, None, False))
    out += [("plain_u8", "f32", "14", False), ("plain_u8", "split_f16", "14", False), ("plain_u8", "f32", None, True)]
    return out


@pytest.mark.parametrize("build,precision,fork,host", _interleaved_params(),
                         ids=[f"{b}:{p}" + (f":fork{f}" if f else "") + (":host" if h else "") for b, p, f, h in _interleaved_params()])
def test_interleaved_geometries(make, weights, stream, build, precision, fork, host):
    """Graphs of A = 37x75 and B = 30x90 on one context, between eager calls of the other shape.  The feature maps of both lie in one
    allocation, and where one shape has its zero border the other has interior: a replay must clear its own border, because the host
    cannot know which shape ran last on the device -- and an eager call after a replay must, for the same reason.  The forced fork adds
    the second workspace, which tracks a geometry of its own; `host` a host-pointer call of B between the replays.  Every result is the
    eager result of its shape and input, from the context's first calls (before any capture)."""
    import torch
    eng = make(3, precision)
    eng.set_experiment("fork", fork or "")
    b = so.Builders(eng, weights[3])
    ca, cb = getattr(b, build)(h=A[0], w=A[1]), getattr(b, build)(h=B[0], w=B[1])
    # the largest shape first; then every shape and input eagerly, before any capture: nothing grows from here on
    want = {("A", "real"): gc.eager(ca, stream, ca.real), ("B", "real"): gc.eager(cb, stream, cb.real),
            ("A", "decoy"): gc.eager(ca, stream, ca.decoy), ("B", "decoy"): gc.eager(cb, stream, cb.decoy)}
    assert gc.differs(want["A", "real"], want["A", "decoy"]) and gc.differs(want["B", "real"], want["B", "decoy"])
    host_px = host_want = None
    if host:
        host_px = so._u8(61, 1, B[0], B[1])
        host_want = eng.upscale_rgba8(host_px)
    # the last eager call before the capture is of A: the host believes the maps are A's, so the captured call queues no clear of its own
    # accord (after a call of B it would: a change of geometry)
    assert not gc.differs(gc.eager(ca, stream, ca.real), want["A", "real"])
    failed, graphs = [], {}

    def step(what, shape, which):
        case = ca if shape == "A" else cb
        src = case.real if which == "real" else case.decoy
        got = gc.replay(case, graphs[shape], stream, src) if what == "replay" else gc.eager(case, stream, src)
        d = gc.differs(got, want[shape, which])
        if d:
            failed.append(f"step {len(steps_done)} ({what} {shape} on {which}): {d}")
        steps_done.append((what, shape, which))
    steps_done = []
    try:
        ca.load(ca.decoy)
        graphs["A"] = gc.capture(ca, stream)
        step("replay", "A", "real")
        step("eager", "B", "decoy")
        step("replay", "A", "decoy")
        step("eager", "B", "real")
        if host:
            got = eng.upscale_rgba8(host_px)
            if not np.array_equal(got, host_want):
                failed.append("the host-pointer call of B between two replays of A differs from itself before the capture")
            step("replay", "A", "real")
        cb.load(cb.decoy)
        graphs["B"] = gc.capture(cb, stream)
        step("replay", "A", "real")
        step("replay", "B", "decoy")
        step("replay", "A", "decoy")
        step("replay", "B", "real")
        step("eager", "A", "real")
        if fork:
            assert eng.last_plan()["fork"][0][0], eng.get_experiment("plan")
        if precision == "split_f16":
            eng.check_domain()
    finally:
        graphs.clear()
        pygc.collect()
        torch.cuda.synchronize()
    assert not failed, f"{build}:{precision}: " + "; ".join(failed)
    EXTRA[f"interleaved {build}:{precision}" + (f":fork{fork}" if fork else "") + (":host" if host else "")] = f"{len(steps_done)} steps"


# ---- (c) one graph of many calls ---------------------------------------------------------------------------------------------------------------
TRAIN = ["border_u8", "sized", "alpha", "ensemble_u8", "upscale_u16", "upscale_yuv", "valid", "backprop"]


def test_one_graph_of_many_calls(make, weights, stream):
    """Eight composed calls that share the context's scratch (each leaves its buffers to the next) in ONE capture, replayed three times on
    changing inputs: every call's result is that of the same sequence made eagerly on a second context."""
    import torch
    ref, eng = make(3), make(3)
    wants = {}
    for e in (ref, eng):   # the reference; and the context under test, warm for every call of the train
        cases = [getattr(so.Builders(e, weights[3]), name)() for name in TRAIN]
        for which in ("decoy", "real"):
            for name, case in zip(TRAIN, cases):
                got = gc.eager(case, stream, getattr(case, which))
                if e is ref:
                    wants[name, which] = got
    for case in cases:
        case.load(case.decoy)
        case.fill_outs(so.SENTINELS[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for case in cases:
            case.run(stream)
    failed = []
    try:
        torch.cuda.synchronize()
        assert all(bool((so._bytes(t) == so.SENTINELS[0]).all()) for case in cases for t in case.outs), "capturing ran something"
        for k, which in enumerate(("real", "decoy", "real")):
            with torch.cuda.stream(stream):
                for case in cases:
                    case.load(getattr(case, which))
                    case.fill_outs(so.SENTINELS[1])
                g.replay()
            torch.cuda.synchronize()
            for name, case in zip(TRAIN, cases):
                d = gc.differs(case.written, wants[name, which])
                if d:
                    failed.append(f"replay {k} ({which}), {name}: {d}")
    finally:
        del g
        torch.cuda.synchronize()
    assert not failed, "; ".join(failed)
    EXTRA["one graph of many calls"] = f"{len(TRAIN)} calls, 3 replays"


# ---- (d) a cold call inside a capture --------------------------------------------------------------------------------------------------------------
def test_cold_call_inside_a_capture(make, weights, stream):
    """A call that would have to allocate while its stream is capturing returns SR_E_INVALID and does nothing: the output is untouched,
    no device memory is taken or given back, the capture goes on and ends cleanly, its replay is right, and the context is as good as
    before -- the same call made eagerly afterwards (once the graph is destroyed) works."""
    import torch
    from rusty_sr_amd import _lib
    ref, eng = make(3), make(3)
    b = so.Builders(eng, weights[3])
    warm, cold = b.plain_u8(), b.plain_u8(h=COLD[0], w=COLD[1])
    want, _, _ = so.reference(warm, stream)
    cold_want = gc.eager(so.Builders(ref, weights[3]).plain_u8(h=COLD[0], w=COLD[1]), stream, cold.real)
    cold.load(cold.real)
    cold.fill_outs(so.SENTINELS[0])
    warm.load(warm.decoy)
    warm.fill_outs(so.SENTINELS[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        free0 = torch.cuda.mem_get_info()[0]   # (around the refused call alone: instantiating a graph may take device memory of its own)
        refused = _status(lambda: cold.run(stream))
        free1 = torch.cuda.mem_get_info()[0]
        after = _status(lambda: warm.run(stream))
    try:
        torch.cuda.synchronize()
        assert refused == _lib.SR_E_INVALID and after == _lib.SR_OK, (refused, after)
        assert free1 == free0, "the refused call allocated or freed"
        assert bool((so._bytes(cold.outs[0]) == so.SENTINELS[0]).all()) and bool((so._bytes(warm.outs[0]) == so.SENTINELS[0]).all())
        assert not gc.differs(gc.replay(warm, g, stream, warm.real), want)
        assert bool((so._bytes(cold.outs[0]) == so.SENTINELS[0]).all()), "the replay wrote the refused call's output"
    finally:
        del g   # only now may the context grow
        pygc.collect()
        torch.cuda.synchronize()
    assert not gc.differs(gc.eager(cold, stream, cold.real), cold_want)
    assert not gc.differs(gc.eager(warm, stream, warm.real), want)
    EXTRA["cold call inside a capture"] = "refused, capture valid, eager call afterwards right"


def test_first_use_tables_inside_a_capture(make, weights, stream):
    """The tables that are uploaded synchronously on their first use (the degradation's, the validation pass's): a first use inside a
    capture is refused like a cold shape, and works afterwards.  The parameter-free graphs build their quantiser table in sr_create, not
    on first use: the bilinear graph's first u8 call needs nothing and is simply recorded."""
    import torch
    from rusty_sr_amd import _lib
    ref, eng = make(3), make(3)
    b, rb = so.Builders(eng, weights[3]), so.Builders(ref, weights[3])
    warm, degrade, valid = b.plain_u8(), b.degrade(), b.valid()
    want, _, _ = so.reference(warm, stream)
    degrade_want, valid_want = gc.eager(rb.degrade(), stream, degrade.real), gc.eager(rb.valid(), stream, valid.real)
    bil, bil_ref = make(3, graph="bilinear"), make(3, graph="bilinear")
    bcase = so.Builders(bil, ()).plain_u8()
    bil_want = gc.eager(so.Builders(bil_ref, ()).plain_u8(), stream, bcase.real)
    for case in (warm, degrade, valid, bcase):
        case.load(case.real)
        case.fill_outs(so.SENTINELS[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        free0 = torch.cuda.mem_get_info()[0]
        got = [_status(lambda: case.run(stream)) for case in (degrade, valid)]
        free1 = torch.cuda.mem_get_info()[0]
        got += [_status(lambda: case.run(stream)) for case in (warm, bcase)]
    try:
        torch.cuda.synchronize()
        assert got == [_lib.SR_E_INVALID, _lib.SR_E_INVALID, _lib.SR_OK, _lib.SR_OK], got
        assert free1 == free0, "a refused call allocated or freed"
        assert all(bool((so._bytes(t) == so.SENTINELS[0]).all()) for case in (degrade, valid, warm, bcase) for t in case.outs)
        with torch.cuda.stream(stream):
            g.replay()
        torch.cuda.synchronize()
        assert not gc.differs(warm.written, want) and not gc.differs(bcase.written, bil_want)
        assert all(bool((so._bytes(t) == so.SENTINELS[0]).all()) for case in (degrade, valid) for t in case.outs)
    finally:
        del g
        pygc.collect()
        torch.cuda.synchronize()
    assert not gc.differs(gc.eager(degrade, stream, degrade.real), degrade_want)
    assert not gc.differs(gc.eager(valid, stream, valid.real), valid_want)
    EXTRA["first-use tables inside a capture"] = "degrade, validation refused; bilinear u8 recorded (its table is sr_create's)"


# ---- (e) the domain flag -----------------------------------------------------------------------------------------------------------------------
def test_domain_flag_under_replay(make, stream):
    """sr_check_domain after a replay reports what the replayed kernels saw.  The twins are tests/domain_cases.py's input-boundary pair
    -- one sample just below 65504, or at it -- because the legs of its node cases differ by their PARAMETERS, which a graph does not
    survive (contract point 3): captured on the inside twin, the graph raises the flag when it is replayed on the outside one, and
    not on the inside one, whose bytes are the eager call's."""
    import torch
    import rusty_sr_amd as r
    import domain_cases as dc
    from rusty_sr_amd import _lib
    eng = r.Engine(dc.boundary_params(), device=0, factor=3, precision="split_f16")
    try:
        under, over = dc.boundary_image("below"), dc.boundary_image("at")
        b = so.Builders(eng, dc.boundary_params())
        case = b.simple(lambda i, o, s: eng.upscale_f32_dev(i[0], out=o[0], stream=s), (under, over), (1, 3 * dc.H, 3 * dc.W, 3), "float32")
        want = gc.eager(case, stream, case.real)
        assert _status(eng.check_domain) == _lib.SR_OK
        case.load(case.real)
        g = gc.capture(case, stream)
        try:
            torch.cuda.synchronize()
            assert _status(eng.check_domain) == _lib.SR_OK, "capturing ran something"
            gc.replay(case, g, stream, case.decoy)
            assert _status(eng.check_domain) == _lib.SR_E_DOMAIN
            got = gc.replay(case, g, stream, case.real)
            assert _status(eng.check_domain) == _lib.SR_OK
            assert not gc.differs(got, want)
        finally:
            del g
            torch.cuda.synchronize()
    finally:
        eng.close()
    EXTRA["domain flag under replay"] = "raised by the replay on the outside twin alone"


# ---- (f) the fork tuner ------------------------------------------------------------------------------------------------------------------------
def test_fork_tuner_takes_no_sample_from_a_captured_call(make, stream):
    """A shape inside the tuner's range (232x320 LR on 256 CUs: 290 tiles, 0.57 rounds), captured while the tuner has not decided: the
    graph is the rule's plan, its bytes the undivided pass's, the tuner's record is what it was, and ten fenced eager calls afterwards
    measure and settle as if nothing had been captured."""
    import torch
    eng = make(3)
    cus = eng.device_info()["compute_units"]
    h, w = max(64, (232 * cus // 256 + 7) // 8 * 8), 320
    eng.set_experiment("forktune", "1")
    eng.reserve(1, h, w)
    px = torch.from_numpy(so._u8(71, 1, h, w)).cuda()
    px2 = torch.from_numpy(so._u8(72, 1, h, w)).cuda()
    src, out = torch.empty_like(px), torch.empty((1, 3 * h, 3 * w, 4), dtype=torch.uint8, device="cuda")
    eng.set_experiment("fork", "0")
    want, want2 = eng.upscale_rgba8_dev(px), eng.upscale_rgba8_dev(px2)
    torch.cuda.synchronize()
    eng.set_experiment("fork", "")
    before = eng.get_experiment("forktune")
    assert before == "", before   # (a forced plan is not the tuner's business: it has not met the shape)
    src.copy_(px)
    out.fill_(so.SENTINELS[0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        eng.upscale_rgba8_dev(src, out=out, stream=stream)
    try:
        torch.cuda.synchronize()
        assert bool((out == so.SENTINELS[0]).all()), "capturing ran something"
        assert eng.last_plan()["fork"] == [(False, 0, 0)], eng.get_experiment("plan")   # 0.57 rounds: the rule's plan is the undivided pass
        for a, b in ((px2, want2), (px, want)):
            with torch.cuda.stream(stream):
                src.copy_(a)
                g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, b)
        assert eng.get_experiment("forktune") == before, "the captured call or its replays left a sample"
    finally:
        del g
        torch.cuda.synchronize()
    for k in range(10):
        assert torch.equal(eng.upscale_rgba8_dev(px), want), k
        torch.cuda.synchronize()
    lines = [l.split() for l in eng.get_experiment("forktune").splitlines()]
    mine = [l for l in lines if l[0] == f"{h}x{w}+0+0" and l[2] == "u8"]
    assert len(mine) == 1 and mine[0][3] in ("undivided", "forked"), lines
    assert float(mine[0][4]) > 0 and float(mine[0][5]) > 0
    EXTRA["fork tuner"] = f"{h}x{w}: no sample from the captured call, settled afterwards as {mine[0][3]}"


# ---- (g) the coverage table --------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_was_captured():
    """Prints entry point x legs that ran.  When the whole module ran, every prototype of include/srhip.h with a `void* stream` has a row
    that passed."""
    by_entry = {}
    for row in gc.ROWS:
        if row["id"] in RESULTS:
            by_entry.setdefault(row["entry"], []).append(RESULTS[row["id"]])
    for entry in so.stream_prototypes():
        ran = by_entry.get(entry, [])
        legs = [leg for leg in gc.LEGS if any(leg in r for r in ran)]
        print(f"{entry:42s} rows {len(ran):2d}  legs {' '.join(legs) if legs else '-'}")
    for i, reason in gc.NOT_CAPTURED.items():
        print(f"not captured: {i}: {reason}")
    for name, line in EXTRA.items():
        print(f"{name:52s} {line}")
    print(f"the module took {time.perf_counter() - T0:.1f} s for {len(RESULTS)} rows and {len(EXTRA)} further tests")
    if len(RESULTS) == len(gc.ROWS):
        assert set(by_entry) == set(so.stream_prototypes())
