"""Stage 2 of the exact mode with half of conv5 as Winograd F(2,3) rows (include/srhip_experimental.h, the "wino" switch): "" (the
default) runs conv5's input channels 0-15 as Winograd rows and 16-31 as direct taps on the pairs, "3" both halves as Winograd rows (a
measurement setting), "2" conv5 direct as before this form existed.  Every setting is held to the exact mode's bar against the f64
oracle; under "" and "3" every kernel form and tile class of stage 2 gives the same bits; "2" reproduces the digests recorded from the
build before this form (tests/golden/wino_conv5_parent_digests.json); a non-finite input pixel reaches the same output pixels as in
the direct form; the split-half mode does not depend on the switch at all."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, synth_u8
from test_gpu_wino_stage2 import FORMS, TIGHT, _stage2_cell

pytestmark = pytest.mark.gpu

DIGEST_SHAPES = ((21, 37, 53), (22, 268, 1024))  # (seed, h, w) of the two recorded inputs
DIGESTS = os.path.join(GOLDEN, "wino_conv5_parent_digests.json")


def _reset(eng):
    for k in ("pipe", "th", "tail", "wino"):
        eng.set_experiment(k, "")


def parent_digests(eng):
    """SHA-256 of stage 2's feature map and of the f32 output under "wino" = "2", for the recorded inputs (one image each, one launch per
    stage).  The committed file holds what the build before the conv5 form gave."""
    out = {}
    eng.set_experiment("fork", "0")
    eng.set_experiment("wino", "2")
    eng.set_pipeline(False)  # one chunk per host call: the feature map read back is the whole image's
    for seed, h, w in DIGEST_SHAPES:
        y = eng.upscale_f32(oracle.img_to_data(synth_u8(seed, 1, h, w)))
        out[f"{seed}:{h}x{w}"] = {"l2": hashlib.sha256(np.ascontiguousarray(eng.read_feature(2, h, w)).tobytes()).hexdigest(),
                                  "out": hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()}
    eng.set_pipeline(True)
    eng.set_experiment("wino", "")
    return out


@pytest.fixture(scope="module")
def engine(params):
    import rusty_sr_amd as r
    eng = r.Engine(params["imagenet"], device=0, precision="f32")
    eng.set_experiment("fork", "0")  # (one launch per stage: the plan record names stage 2's one cell)
    yield eng
    eng.close()


@pytest.mark.parametrize("shape", ((1, 37, 53), (2, 117, 301)), ids=lambda s: "x".join(map(str, s)))
def test_every_conv5_setting_within_the_exact_bar(engine, params, shape):
    n, h, w = shape
    x = oracle.img_to_data(synth_u8(11 + h, n, h, w))
    want = oracle.forward(params["imagenet"], x, f64=True)
    _reset(engine)
    for s in ("2", "3", ""):
        engine.set_experiment("wino", s)
        err = float(np.abs(engine.upscale_f32(x).astype(np.float64) - want).max())
        print(f"wino={s!r} {shape}: max |gpu - f64 oracle| = {err:.3e}")
        assert err < TIGHT, (s, shape, err)
    _reset(engine)


@pytest.mark.parametrize("setting", ("", "3"), ids=lambda s: s or "default")
def test_forms_and_tile_classes_are_bit_identical(engine, setting):
    h, w = 268, 1024
    x = oracle.img_to_data(synth_u8(3, 1, h, w))
    outs, l2 = {}, {}
    for cell, sw in FORMS.items():
        _reset(engine)
        engine.set_pipeline(False)  # one chunk per host call: the forced switches apply to the one launch of each stage
        engine.set_experiment("wino", setting)
        for k, v in sw.items():
            engine.set_experiment(k, v)
        outs[cell] = engine.upscale_f32(x)
        assert _stage2_cell(engine) == cell, (cell, engine.get_experiment("plan"))
        l2[cell] = engine.read_feature(2, h, w)
    _reset(engine)
    engine.set_pipeline(True)
    ref = "pipe/8"
    for cell in FORMS:
        np.testing.assert_array_equal(l2[cell], l2[ref], err_msg=cell)
        np.testing.assert_array_equal(outs[cell], outs[ref], err_msg=cell)


def test_setting_2_reproduces_the_build_before_the_conv5_form(engine):
    with open(DIGESTS) as f:
        want = json.load(f)
    _reset(engine)
    got = parent_digests(engine)
    _reset(engine)
    assert got == want


def test_non_finite_pixels_reach_what_they_reach_in_the_direct_form(engine):
    h, w = 24, 40
    x = oracle.img_to_data(synth_u8(9, 1, h, w)).astype(np.float32)
    x[0, 5, 6, 1] = np.nan
    x[0, 17, 31, 0] = np.inf
    _reset(engine)
    bad = {}
    for s in ("", "0"):
        engine.set_experiment("wino", s)
        bad[s] = ~np.isfinite(engine.upscale_f32(x)).all(axis=3)
    _reset(engine)
    assert bad["0"].any() and not bad["0"].all()
    np.testing.assert_array_equal(bad[""], bad["0"])


def test_split_half_mode_does_not_depend_on_the_switch(params):
    import rusty_sr_amd as r
    eng = r.Engine(params["imagenet"], device=0, precision="split_f16")
    try:
        x = oracle.img_to_data(synth_u8(4, 1, 268, 1024))
        outs = {}
        for s in ("0", "1", "2", "3", ""):
            eng.set_experiment("wino", s)
            outs[s] = eng.upscale_f32(x)
        for s in outs:
            np.testing.assert_array_equal(outs[s], outs["0"], err_msg=s)
    finally:
        eng.close()
