"""The "wino" switch of the exact mode (include/srhip_experimental.h): "0" all stages direct, "1" stage 1 as Winograd F(2,3) rows,
"" / "2" (the default) stages 1 and 2.  Every setting is held to the exact mode's bar against the f64 oracle, at 1080p width and at
geometries whose width is no multiple of 32 and whose height no multiple of 8; under the default every kernel form and tile class of
stage 2 gives the same bits (sr_kernels.hip half_steps_wino / half_steps_pairs: one accumulation order); the split-half mode does not
depend on the switch at all."""
import numpy as np
import pytest

import oracle
from conftest import synth_u8

pytestmark = pytest.mark.gpu

TIGHT = 2e-5  # the exact mode's bar against the f64 oracle (tests/test_gpu_kernel_matrix.py)
SETTINGS = ("0", "1", "2", "")
SHAPES = ((1, 544, 1920), (1, 37, 53), (1, 83, 250), (2, 117, 301))
FORMS = {  # stage 2's cell -> the switches that force it (sr_set_experiment); 268x1024 is >= 2 rounds of 8-row tiles
    "first/4": {"pipe": "none", "th": "4"},
    "first/8": {"pipe": "none", "th": "8"},
    "pipe/4": {"pipe": "all", "th": "4"},
    "pipe/8": {"pipe": "all", "th": "8"},
    "pipe/8+4": {"pipe": "all", "tail": "1"},
}


@pytest.fixture(scope="module")
def engine(params):
    import rusty_sr_amd as r
    eng = r.Engine(params["imagenet"], device=0, precision="f32")
    eng.set_experiment("fork", "0")  # (one launch per stage: the plan record names stage 2's one cell)
    yield eng
    eng.close()


def _reset(eng):
    for k in ("pipe", "th", "tail", "wino"):
        eng.set_experiment(k, "")


def _stage2_cell(eng):
    l2 = [l for l in eng.last_plan()["launches"] if l["st"] == 2]
    assert len(l2) == 1 and l2[0]["count"] == 1, eng.get_experiment("plan")
    l = l2[0]
    return f"{l['form']}/" + ("8+4" if l["ty8"] and l["ty4"] else "8" if l["ty8"] else "4")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_setting_within_the_exact_bar(engine, params, shape):
    n, h, w = shape
    px = synth_u8(11 + h, n, h, w)
    x = oracle.img_to_data(px)
    want = oracle.forward(params["imagenet"], x, f64=True)
    _reset(engine)
    for s in SETTINGS:
        engine.set_experiment("wino", s)
        got = engine.upscale_f32(x)
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err < TIGHT, (s, shape, err)
    _reset(engine)


def test_default_forms_and_tile_classes_are_bit_identical(engine):
    h, w = 268, 1024
    px = synth_u8(3, 1, h, w)
    x = oracle.img_to_data(px)
    outs, l2 = {}, {}
    for cell, sw in FORMS.items():
        _reset(engine)
        engine.set_pipeline(False)  # one chunk per host call: the forced switches apply to the one launch of each stage
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


def test_split_half_mode_does_not_depend_on_the_switch(params):
    import rusty_sr_amd as r
    eng = r.Engine(params["imagenet"], device=0, precision="split_f16")
    try:
        x = oracle.img_to_data(synth_u8(4, 1, 268, 1024))
        outs = {}
        for s in SETTINGS:
            eng.set_experiment("wino", s)
            outs[s] = eng.upscale_f32(x)
        for s in SETTINGS:
            np.testing.assert_array_equal(outs[s], outs["0"], err_msg=s)
    finally:
        eng.close()
