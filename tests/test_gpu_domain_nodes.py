"""The split-half mode's domain check ("domain checked, never clamped": include/srhip.h sr_set_precision / sr_check_domain) held to the
oracle at every node and through every plan, on the cases of tests/domain_cases.py: ONE value of one node -- f, l1, l2 or l3, at the
first pixel, the last pixel or a tile seam, in the first or the last channel -- at 1.03 x 65504 (the over leg: SR_E_DOMAIN once, then
SR_OK) or at 0.97 x 65504 (the under leg: SR_OK, computed in split arithmetic and right), and one input sample at 65504, -65504 or
the float just below.  tests/test_domain_cases_cpu.py has shown on the oracle alone that the cases are what they claim.

  (a) the truth table: every case, both legs, through sr_upscale_f32_dev + sr_check_domain under the default plan, both tile heights,
      both kernel forms and their four crossings
  (b) the under leg is split arithmetic and within the project's bar for large values, node by node (the measured errors:
      profiles/domain_nodes.txt)
  (c) the over leg through the host-pointer calls: the exact-f32 engine's bits under every host plan, a batch, several contexts;
      the under leg through the same calls: the split-half kernels' bits
  (d) the over leg through the other device forms: bands, forked calls, the ensemble, the transparency and validation passes, sharded calls
  (e) no stale positives: nothing of an overflowing call at a larger geometry flags a later, smaller, ordinary call

37 x 75 images (partial tiles on both axes); one split-half engine per factor, sr_set_params between cases."""
import numpy as np
import pytest

import domain_cases as dc
import oracle
from conftest import synth_u8

pytestmark = pytest.mark.gpu

H, W = dc.H, dc.W
MASK = 0b10011  # members 0, 1 and the axis-swapping member 4
FORMS = {
    "default": {},
    "th=4": {"th": "4"}, "th=8": {"th": "8"},
    "pipe=none": {"pipe": "none"}, "pipe=all": {"pipe": "all"},
    "first/4": {"pipe": "none", "th": "4"}, "first/8": {"pipe": "none", "th": "8"},
    "pipe/4": {"pipe": "all", "th": "4"}, "pipe/8": {"pipe": "all", "th": "8"},
}
SWITCHES = ("th", "pipe", "fork", "bands", "rows")
ROWS3 = [r for r in dc.TABLE if r[3] == 3]
ROWS3_B31 = [r for r in ROWS3 if r[2] == 31]


class Pool:
    """The engines of the module: per factor one split-half engine and one exact-f32 engine, further split-half contexts on demand."""

    def __init__(self):
        self.split, self.f32, self.more = {}, {}, {}

    def _new(self, factor, precision):
        import rusty_sr_amd as r
        return r.Engine(dc.base_params(factor), device=0, factor=factor, precision=precision)

    def get(self, factor=3):
        if factor not in self.split:
            self.split[factor] = self._new(factor, "split_f16")
            self.f32[factor] = self._new(factor, "f32")
        reset(self.split[factor])
        return self.split[factor], self.f32[factor]

    def contexts(self, key, n):
        """n further split-half contexts of factor 3 under a name of their own (a communicator, once made, stays with its contexts)"""
        if key not in self.more:
            self.more[key] = [self._new(3, "split_f16") for _ in range(n)]
        return self.more[key]

    def close(self):
        for e in list(self.split.values()) + list(self.f32.values()) + [e for es in self.more.values() for e in es]:
            e.close()


@pytest.fixture(scope="module")
def pool():
    p = Pool()
    yield p
    p.close()


def reset(eng):
    for k in SWITCHES:
        eng.set_experiment(k, "")
    eng.set_pipeline(True)


def apply(eng, form):
    for k in ("th", "pipe"):
        eng.set_experiment(k, FORMS[form].get(k, ""))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sync():
    import torch
    torch.cuda.synchronize()


def flagged(eng, wait=True):
    """sr_check_domain once the device is idle (wait=False: as things are): True for SR_E_DOMAIN, and the report is then gone"""
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    if wait:
        sync()
    try:
        eng.check_domain()
    except r.SrError as e:
        assert e.status == _lib.SR_E_DOMAIN
        eng.check_domain()  # reported once
        return True
    return False


def legs(row):
    node, pos, b, factor = row
    return [(leg, dc.case(node, pos, b, leg, factor)) for leg in dc.LEGS]


# ---- (a) the truth table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", dc.TABLE, ids=dc.table_id)
def test_truth_table(pool, row):
    eng, _ = pool.get(row[3])
    wrong = []
    for leg, c in legs(row):
        eng.set_params(c.params)
        x = dev(c.x)
        for form in FORMS:
            apply(eng, form)
            eng.upscale_f32_dev(x)
            if flagged(eng) != (leg == "over"):
                wrong.append((c.id, form))
    assert not wrong, wrong


def test_truth_table_of_the_input_boundary(pool):
    eng, _ = pool.get(3)
    eng.set_params(dc.boundary_params())
    wrong = []
    for which, (_, leaves) in dc.BOUNDARY.items():
        x = dev(dc.boundary_image(which))
        for form in FORMS:
            apply(eng, form)
            eng.upscale_f32_dev(x)
            if flagged(eng) != leaves:
                wrong.append((which, form))
    assert not wrong, wrong


# ---- (b) the under leg: split arithmetic, and right --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", dc.TABLE, ids=dc.table_id)
def test_under_leg_is_split_arithmetic_and_right(pool, row):
    """|gpu - t64| <= 1e-4 max|t64| of every node and of the output: the project's rule for large values (tests/test_gpu_domain.py,
    TOL * max|want|), nothing measured here went into it.  The host call returns the device call's bits and not the exact-f32 engine's:
    no recompute happened, the values of 3e4 .. 6.4e4 were carried as half pairs."""
    node, pos, b, factor = row
    c = dc.case(node, pos, b, "under", factor)
    eng, f32 = pool.get(factor)
    eng.set_params(c.params)
    f32.set_params(c.params)
    eng.set_pipeline(False)          # one chunk, one band: read_feature sees the whole image
    eng.set_experiment("fork", "0")
    got = eng.upscale_f32(c.x)
    failed = []
    for k, key in enumerate(dc.NODES):
        t64 = c.t64[key]
        top = float(np.abs(t64).max())
        err = float(np.abs(eng.read_feature(k, H, W).astype(np.float64) - t64).max())
        ref = float(np.abs(c.t32[key].astype(np.float64) - t64).max())
        print(f"domain node {c.id} {key}: max|t64| {top:.6g}  |t32 - t64| {ref:.3e}  |gpu - t64| {err:.3e}  relative {err / top:.2e}")
        if not err <= dc.OUT_TOL * top:
            failed.append((key, err, top))
    top = float(np.abs(c.o64).max())
    err = float(np.abs(got.astype(np.float64) - c.o64).max())
    ref = float(np.abs(c.o32.astype(np.float64) - c.o64).max())
    print(f"domain node {c.id} out: max|t64| {top:.6g}  |t32 - t64| {ref:.3e}  |gpu - t64| {err:.3e}  relative {err / top:.2e}")
    if not err <= dc.OUT_TOL * top:
        failed.append(("output", err, top))
    assert not failed, (c.id, failed)
    assert not flagged(eng)
    out = eng.upscale_f32_dev(dev(c.x))
    assert not flagged(eng)
    np.testing.assert_array_equal(out.cpu().numpy(), got, err_msg="the host call did not return the split-half kernels' bits")
    assert not np.array_equal(got, f32.upscale_f32(c.x)), "the two modes give the same bits: the comparison above proves nothing"


# ---- (c) the over leg through the host-pointer calls ---------------------------------------------------------------------------------------
HOST_PLANS = {  # name -> (pipeline, switches, the band rows the plan record must show)
    "one chunk": (False, {}, None),
    "bands=2": (True, {"bands": "2"}, 2),
    "bands=3": (True, {"bands": "3"}, 2),          # (37 rows hold two bands of 2 x 7 rows and more: the planner's own limit)
    "rows 12,12,13": (True, {"rows": "12,12,13"}, 3),
    "rows =12,12,13": (True, {"rows": "=12,12,13"}, 3),   # ... three on alternating streams
}


def ordinary_u8():
    return np.ascontiguousarray(synth_u8(901, 1, H, W) // 8)


@pytest.mark.parametrize("row", ROWS3, ids=dc.table_id)
def test_over_leg_host_calls_are_the_exact_engines_bits(pool, row):
    node, pos, b, factor = row
    c = dc.case(node, pos, b, "over", factor)
    eng, f32 = pool.get(factor)
    eng.set_params(c.params)
    f32.set_params(c.params)
    want32, want8 = f32.upscale_f32(c.x), f32.upscale_rgba8(c.px)
    px0 = ordinary_u8()
    x0 = oracle.img_to_data(px0)
    split0 = eng.upscale_f32_dev(dev(x0)).cpu().numpy()     # the split-half mode's bits of an ordinary image on these parameters
    assert not flagged(eng)
    assert not np.array_equal(split0, f32.upscale_f32(x0))
    for name, (pipeline, switches, nbands) in HOST_PLANS.items():
        reset(eng)
        eng.set_pipeline(pipeline)
        for k, v in switches.items():
            eng.set_experiment(k, v)
        got32 = eng.upscale_f32(c.x)
        host = eng.last_plan()["host"]   # (the split-half pass's plan and the exact pass's)
        assert 1 <= len(host) <= 2 and all(k == "one" if nbands is None else len(sizes) == nbands for k, sizes, _ in host), (name, host)
        np.testing.assert_array_equal(got32, want32, err_msg=f"{c.id} {name} f32")
        eng.check_domain()  # the synchronous call has dealt with it
        np.testing.assert_array_equal(eng.upscale_rgba8(c.px), want8, err_msg=f"{c.id} {name} u8")
        eng.check_domain()
        np.testing.assert_array_equal(eng.upscale_f32(x0), split0, err_msg=f"{c.id} {name}: not back in the split-half mode")
        eng.check_domain()
    # a batch of three in which only the last image carries P
    reset(eng)
    batch = np.concatenate([x0, oracle.img_to_data(synth_u8(902, 1, H, W) // 8), c.x])
    for pipeline in (True, False):
        eng.set_pipeline(pipeline)
        np.testing.assert_array_equal(eng.upscale_f32(batch), f32.upscale_f32(batch), err_msg=f"{c.id} batch pipeline={pipeline}")
        eng.check_domain()
        np.testing.assert_array_equal(eng.upscale_f32(x0), split0)


@pytest.mark.parametrize("row", ROWS3_B31, ids=dc.table_id)
def test_over_leg_over_several_contexts(pool, row):
    """sr_upscale_*_multi: every context computes a share of the rows from the rows themselves +- 7; a share whose extended rows hold P
    has left the domain and is the exact-f32 engine's, the others are the split-half mode's.  sr_upscale_*_batch_multi: image i goes to
    context i mod k; the context that got the image with P recomputes its images.  No context is left flagged."""
    import rusty_sr_amd as r
    node, pos, b, factor = row
    c = dc.case(node, pos, b, "over", factor)
    eng, f32 = pool.get(factor)
    engs = [eng] + pool.contexts("multi", 2)
    for e in engs:
        reset(e)
        e.set_params(c.params)
    f32.set_params(c.params)
    want = {"f32": f32.upscale_f32(c.x)[0], "u8": f32.upscale_rgba8(c.px)[0]}
    split = {"f32": eng.upscale_f32_dev(dev(c.x))[0].cpu().numpy(), "u8": eng.upscale_rgba8_dev(dev(c.px))[0].cpu().numpy()}
    assert flagged(eng)
    py = c.P[0]
    for k in (2, 3):
        for io, src in (("f32", c.x[0]), ("u8", c.px[0])):
            got = r.upscale_multi(engs[:k], src)
            shares = [e.last_plan()["host"] for e in engs[:k]]
            shares = [s[0][2] for s in shares if s]
            assert len(shares) >= 2 and all(s is not None for s in shares) and sum(hi - lo for lo, hi in shares) == H, shares
            for lo, hi in shares:
                holds = lo - 7 <= py < hi + 7
                ref = want[io] if holds else split[io]
                np.testing.assert_array_equal(got[factor * lo:factor * hi], ref[factor * lo:factor * hi],
                                              err_msg=f"{c.id} {io} on {k}: rows {lo}:{hi} {'hold' if holds else 'do not hold'} P")
            assert not any(flagged(e) for e in engs)
    px0 = ordinary_u8()
    x0 = oracle.img_to_data(px0)
    batch = np.concatenate([x0, oracle.img_to_data(synth_u8(902, 1, H, W) // 8), c.x])
    want_b = f32.upscale_f32(batch)
    split_b = eng.upscale_f32_dev(dev(batch)).cpu().numpy()
    assert flagged(eng)
    for k in (2, 3):
        got = r.upscale_batch_multi(engs[:k], batch)
        for i in range(3):
            ref = want_b if i % k == 2 % k else split_b
            np.testing.assert_array_equal(got[i], ref[i], err_msg=f"{c.id} batch on {k}: image {i}")
        assert not any(flagged(e) for e in engs)
        np.testing.assert_array_equal(r.upscale_batch_multi(engs[:k], batch[:2]), split_b[:2], err_msg="not back in the split-half mode")


@pytest.mark.parametrize("row", ROWS3_B31, ids=dc.table_id)
def test_under_leg_host_calls_stay_in_split_arithmetic(pool, row):
    """The other leg of (c): with the value at 0.97 x 65504 every host plan, the batch and the calls over several contexts return the
    split-half kernels' bits (the device call's), never the exact engine's, and leave nothing to report."""
    import rusty_sr_amd as r
    node, pos, b, factor = row
    c = dc.case(node, pos, b, "under", factor)
    eng, f32 = pool.get(factor)
    engs = [eng] + pool.contexts("multi", 2)
    for e in engs:
        reset(e)
        e.set_params(c.params)
    f32.set_params(c.params)
    batch = np.concatenate([oracle.img_to_data(ordinary_u8()), oracle.img_to_data(synth_u8(902, 1, H, W) // 8), c.x])
    split32, split8 = eng.upscale_f32_dev(dev(batch)).cpu().numpy(), eng.upscale_rgba8_dev(dev(c.px)).cpu().numpy()
    assert not flagged(eng)
    assert not np.array_equal(split32[2], f32.upscale_f32(c.x)[0])
    for name, (pipeline, switches, nbands) in HOST_PLANS.items():
        reset(eng)
        eng.set_pipeline(pipeline)
        for k, v in switches.items():
            eng.set_experiment(k, v)
        np.testing.assert_array_equal(eng.upscale_f32(c.x)[0], split32[2], err_msg=f"{c.id} {name} f32")
        host = eng.last_plan()["host"]
        assert len(host) == 1 and (host[0][0] == "one" if nbands is None else len(host[0][1]) == nbands), (name, host)   # (one pass)
        np.testing.assert_array_equal(eng.upscale_rgba8(c.px), split8, err_msg=f"{c.id} {name} u8")
        eng.check_domain()
    reset(eng)
    np.testing.assert_array_equal(eng.upscale_f32(batch), split32, err_msg=f"{c.id} batch")
    for k in (2, 3):
        np.testing.assert_array_equal(r.upscale_multi(engs[:k], c.x[0]), split32[2], err_msg=f"{c.id} f32 on {k}")
        np.testing.assert_array_equal(r.upscale_multi(engs[:k], c.px[0]), split8[0], err_msg=f"{c.id} u8 on {k}")
        np.testing.assert_array_equal(r.upscale_batch_multi(engs[:k], batch), split32, err_msg=f"{c.id} batch on {k}")
        for e in engs:
            e.check_domain()


# ---- (d) the over leg through the other device forms: the flag ----------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS3, ids=dc.table_id)
def test_other_device_forms_raise_the_flag(pool, row):
    import torch
    node, pos, b, factor = row
    eng, _ = pool.get(factor)
    py = dc.POSITIONS[pos][0]
    # bands (own rows, extended by 7 where the image goes on): P in the band's own rows; and one row outside them, where every node is
    # still computed (the last stage reads l3 one row beyond its own)
    own = {"first": (0, 16), "seam": (8, 24), "last": (21, 37)}[pos]
    bands = {"own rows": own}
    if pos == "seam":
        bands["halo row"] = (16, 30)
    wrong = []
    for leg, c in legs(row):
        eng.set_params(c.params)
        reset(eng)
        x, px = dev(c.x), dev(c.px)

        def expect(what):
            if flagged(eng) != (leg == "over"):
                wrong.append((c.id, what))

        for name, (a, z) in bands.items():
            top, bot = (0 if a == 0 else 7), (0 if z == H else 7)
            assert (a <= py < z) == (name == "own rows") and a - top <= py < z + bot
            eng.upscale_band_f32_dev(x[0, a - top:z + bot].contiguous(), top, bot)
            expect(f"band {name}")
        # a forced fork: the second band's kernels run on the library's other stream; the flag is there once the caller's has drained
        eng.set_experiment("fork", "1")
        side = torch.cuda.Stream()
        for stream in (None, side):
            if stream is None:
                out = eng.upscale_f32_dev(x)
            else:
                with torch.cuda.stream(side):
                    out = eng.upscale_f32_dev(x, stream=side)
            fork = eng.last_plan()["fork"]
            assert len(fork) == 1 and fork[0][0] and fork[0][1] + fork[0][2] == H, fork
            if stream is None:
                expect(f"fork {fork[0][1]},{fork[0][2]}")
            else:
                side.synchronize()   # the caller's stream alone: no device-wide wait before the look
                if flagged(eng, wait=False) != (leg == "over"):
                    wrong.append((c.id, f"fork {fork[0][1]},{fork[0][2]} on a side stream"))
                assert not flagged(eng)
            del out
        eng.set_experiment("fork", "")
        eng.upscale_ensemble_f32_dev(x, MASK)
        expect("ensemble")
        alpha = np.random.default_rng(5).integers(1, 256, (1, H, W, 1), dtype=np.uint8)   # (no pixel transparent: nothing is bled over P)
        eng.upscale_rgba8_alpha_dev(dev(np.concatenate([c.px, alpha], axis=-1)))
        expect("alpha")
        eng.validation_error_pair_dev(px[0], dev(synth_u8(903, 1, factor * H, factor * W)[0]))
        expect("validation pair")
    assert not wrong, wrong
    # P was in the first band of the fork for the first pixel and in the second for the last one
    assert pos == "seam" or (py < fork[0][1]) == (pos == "first")


@pytest.mark.parametrize("n", [2, 3])
def test_sharded_calls_raise_the_owners_flag(pool, n):
    """sr_upscale_sharded_*_all over n contexts of device 0, halos by peer copy, in both halo modes: the context whose band holds P
    reports SR_E_DOMAIN; in the under leg none does.  (A neighbour that recomputes P's rows from its halo may report as well: its
    report is collected, not judged.)"""
    import rusty_sr_amd as r
    from rusty_sr_amd.shard import split_rows
    engs = pool.contexts(f"sharded{n}", n)
    r.comm_init_all(engs, transport="local")
    cuts = split_rows(H, n)
    wrong = []
    for row in ROWS3_B31:
        py = dc.POSITIONS[row[1]][0]
        owner = [a <= py < z for a, z in cuts].index(True)
        for leg, c in legs(row):
            for e in engs:
                e.set_params(c.params)
            for halo in ("input", "layers"):
                for e in engs:
                    e.set_experiment("halo", halo)
                for src in (c.x[0], c.px[0]):
                    r.upscale_sharded_all(engs, [dev(src[a:z]) for a, z in cuts])
                    seen = [flagged(e) for e in engs]
                    if leg == "over" and not seen[owner] or leg == "under" and any(seen):
                        wrong.append((c.id, halo, str(src.dtype), owner, seen))
    assert not wrong, wrong


# ---- (e) no stale positives --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("node", dc.NODES)
def test_nothing_stale_flags_a_later_call(pool, node):
    """An over-leg call at 48 x 96 in which EVERY pixel of the node's channel is beyond the limit leaves saturated halves all over the
    maps.  A smaller image afterwards lives in the top-left corner of the same memory: the lanes of its partial tiles that lie outside
    the image still run the epilogue and its tracking (their stores alone are masked), and must not find anything there."""
    eng, _ = pool.get(3)
    over, under = dc.case(node, "last", 31, "over"), dc.case(node, "last", 31, "under")
    big = synth_u8(904, 1, 48, 96) // 8
    big[..., 0] = 255
    big = dev(oracle.img_to_data(big.astype(np.uint8)))
    small = {
        "ordinary 37x75": oracle.img_to_data(synth_u8(905, 1, H, W)),
        "ordinary 9x13": oracle.img_to_data(synth_u8(906, 1, 9, 13)),
        "ordinary 1x1": oracle.img_to_data(synth_u8(907, 1, 1, 1)),
        "under leg 37x75": under.x,
    }
    assert all(x.max() < 0.9 for name, x in small.items() if name.startswith("ordinary"))   # (R = 1 is what the gain was found for)
    wrong = []
    for form in FORMS:
        apply(eng, form)
        for name, x in small.items():
            eng.set_params(over.params)
            eng.upscale_f32_dev(big)
            assert flagged(eng), (node, form)
            eng.set_params(under.params)
            eng.upscale_f32_dev(dev(x))
            if flagged(eng):
                wrong.append((node, form, name))
    assert not wrong, wrong
