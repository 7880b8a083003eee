"""Inference and backpropagation against the oracle on the parameter families of tests/param_families.py (init, early, wide, tiny,
dim), which tests/test_param_families_cpu.py has shown to be what they claim and well conditioned on the reference: the f32 output
at every factor in both arithmetic modes, every node at factor 3, the Winograd settings and the forced kernel forms on the families
that stress them, the gradient, and sr_set_params from one scale to another.

The bars are multiples of the oracle's own f32 error (|t32 - t64|), not relative to the node: in `tiny` the nodes l1..l3 are ~3e-4
and the oracle's f32 error on them 1e-7, the cancellation in sqrt(z^2 + 1) - 1.  What (b) checks is that no family is worse relative
to the oracle's own error than imagenet.rsr, the family the rest of the suite vouches for; profiles/param_families_errors.txt holds
the measured ratios.

C_NODE is the factor c of the node bar  |gpu - t64| <= c max|t32 - t64| + 1e-7 max(1, max|t64|):  2, the project's own factor
(test_gpu_kernel_matrix._check_f32), except where the control row imagenet.rsr itself needs more -- then twice the control's measured
ratio, rounded up to a power of two, at most 16; see the table for the reasons."""
import numpy as np
import pytest
import torch

import grad_ref
import oracle
import param_families as pf
from test_gpu_backprop import assert_grad_close, gpu_pool, validation_err
from test_gpu_kernel_matrix import FORMS, PRECISIONS, SWITCHES, TOL, _check_u8, _expect_cell, _quantise
from test_gpu_wino_stage2 import _stage2_cell

pytestmark = pytest.mark.gpu

NODE_BAR = 2e-5          # the suite's node bar (test_gpu_parity.test_per_stage_features): 2e-5 max(1, max|node|)
CELLS = ("first/4", "first/8", "pipe/4", "pipe/8")

# (node, mode) -> c.  Calibrated on the control row (imagenet.rsr, both images) alone and then the same for every family.  The control
# row's measured ratios max|gpu - t64| / max|t32 - t64| (profiles/param_families_errors.txt):
#              f     l1    l2    l3
#   f32        1.34  0.95  1.01  1.12     the F(2,3) rows of stages 1 and 2 (l1, l2) do not show above the direct form's error
#   split_f16  1.96  1.63  1.18  1.14     22-bit pairs against a 24-bit significand: below 2 all the same
# None needs more than 2, so every (node, mode) keeps the project's own factor; no entry is raised.
C_NODE = {(k, m): 2 for k in pf.NODES for m in PRECISIONS}


def _engine(name, factor, precision):
    import rusty_sr_amd as r
    return r.Engine(pf.weights(name, factor), device=0, factor=factor, precision=precision)


def _reset(eng):
    for k in SWITCHES + ("wino",):
        eng.set_experiment(k, "")
    eng.set_pipeline(True)


def _check_output(got, o32, o64, what):
    """_check_f32 of tests/test_gpu_kernel_matrix.py with its constants, scaled for outputs above 1"""
    top = max(1.0, float(np.abs(o64).max()))
    assert got.shape == o32.shape
    e32 = float(np.abs(got - o32).max())
    e64 = float(np.abs(got.astype(np.float64) - o64).max())
    ref = float(np.abs(o32.astype(np.float64) - o64).max())
    print(f"output {what}: |gpu - o32| {e32:.3e}  |gpu - o64| {e64:.3e}  |o32 - o64| {ref:.3e}  max|o64| {top:.3g}")
    assert e32 < TOL * top, (what, e32)
    assert e64 <= 2 * ref + 1e-7 * top, (what, e64, ref)


def _check_nodes(eng, name, which, mode, what):
    """read_feature(0..3) of the last call against forward_taps in f64: the suite's hard bar and the bar tied to the reference"""
    t32, t64, _, _ = pf.taps(name, which)
    h, w = pf.node_image(which).shape[1:3]
    failed = []
    for k, key in enumerate(pf.NODES):
        got = eng.read_feature(k, h, w).astype(np.float64)
        top = max(1.0, float(np.abs(t64[key]).max()))
        err = float(np.abs(got - t64[key]).max())
        ref = float(np.abs(t32[key].astype(np.float64) - t64[key]).max())
        print(f"node {what} {key}: |gpu - t64| {err:.3e}  |t32 - t64| {ref:.3e}  ratio {err / ref:.2f}  max|t64| {np.abs(t64[key]).max():.3g}")
        if not err < NODE_BAR * top:
            failed.append((key, "hard bar", err, NODE_BAR * top))
        if not err <= C_NODE[(key, mode)] * ref + 1e-7 * top:
            failed.append((key, "reference bar", err, ref, err / ref))
    assert not failed, (what, failed)


# ---- (a) the output, default plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("factor", pf.FACTORS)
@pytest.mark.parametrize("name", pf.FAMILIES)
def test_output_against_the_oracle(name, factor, precision):
    eng = _engine(name, factor, precision)
    try:
        for which in pf.IMAGES:
            px = pf.image(which, factor)
            o32, o64 = pf.truth(name, factor, which)
            x = oracle.img_to_data(px)
            got32 = eng.upscale_f32(x)
            if precision == "split_f16":
                # none of these families leaves the f16 range.  A host-pointer call that did would have recomputed in exact f32 and left
                # no fault behind; the device call leaves it to sr_check_domain, and its bits are the host call's (one arithmetic)
                dev = eng.upscale_f32_dev(torch.from_numpy(x).cuda())
                torch.cuda.synchronize()
                eng.check_domain()
                np.testing.assert_array_equal(dev.cpu().numpy(), got32, err_msg="the host call did not run the split-half kernels")
            _check_output(got32, o32, o64, f"{name} f{factor} {precision} {which}")
            got8 = eng.upscale_rgba8(px)
            if precision == "split_f16":
                eng.check_domain()
            np.testing.assert_array_equal(got8, _quantise(got32), err_msg="u8 != quantised f32")
            _check_u8(got8, o32)
    finally:
        eng.close()


# ---- (b) the nodes at factor 3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ("imagenet",) + pf.FAMILIES)   # the control row first
def test_nodes_against_the_oracle(name, precision):
    eng = _engine(name, 3, precision)
    try:
        eng.set_pipeline(False)          # one chunk, one band: read_feature sees the whole image
        eng.set_experiment("fork", "0")
        for which in pf.IMAGES:
            _, _, o32, o64 = pf.taps(name, which)
            got = eng.upscale_f32(oracle.img_to_data(pf.node_image(which)))
            _check_nodes(eng, name, which, precision, f"{name} {precision} {which}")
            _check_output(got, o32, o64, f"{name} f3 {precision} {which}[0]")
    finally:
        eng.close()


# ---- (c) Winograd settings and kernel forms on the families that stress them, factor 3 ----------------------------------------------------
@pytest.mark.parametrize("name", ("wide", "early", "dim"))
def test_winograd_settings_in_the_exact_mode(name):
    """"wino": "0" all direct, "1" stage 1 as F(2,3) rows, "2" stages 1 and 2 (conv5 direct), "" the default (half of conv5 as rows),
    "3" all of conv5 as rows.  Every setting within the bars of (a) and (b); under "" and "3" every forced form of stage 2 gives the
    same bits (as tests/test_gpu_wino_conv5.py shows on imagenet.rsr)."""
    eng = _engine(name, 3, "f32")
    try:
        for which in pf.IMAGES:
            x = oracle.img_to_data(pf.node_image(which))
            h, w = x.shape[1:3]
            _, _, o32, o64 = pf.taps(name, which)
            for s in ("0", "1", "2", "3", ""):
                _reset(eng)
                eng.set_pipeline(False)
                eng.set_experiment("fork", "0")
                eng.set_experiment("wino", s)
                got = eng.upscale_f32(x)
                _check_output(got, o32, o64, f"{name} wino={s!r} {which}")
                _check_nodes(eng, name, which, "f32", f"{name} wino={s!r} {which}")
            for s in ("", "3"):
                outs, l2 = {}, {}
                for cell in CELLS:
                    _reset(eng)
                    eng.set_pipeline(False)
                    eng.set_experiment("fork", "0")
                    eng.set_experiment("wino", s)
                    for k, v in FORMS[cell].items():
                        eng.set_experiment(k, v)
                    outs[cell] = eng.upscale_f32(x)
                    assert _stage2_cell(eng) == cell, (cell, eng.get_experiment("plan"))
                    l2[cell] = eng.read_feature(2, h, w)
                for cell in CELLS:
                    np.testing.assert_array_equal(l2[cell], l2["pipe/8"], err_msg=f"{name} wino={s!r} {which} l2 {cell}")
                    np.testing.assert_array_equal(outs[cell], outs["pipe/8"], err_msg=f"{name} wino={s!r} {which} {cell}")
    finally:
        eng.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ("wide", "dim"))
def test_forced_final_stage_cells(name, precision):
    """first/4, first/8, pipe/4, pipe/8 with the plan record asserting what ran: each within (a), and the forms bit-identical to each
    other (test_gpu_parity.test_pipe_form_equals_first_form_bit_for_bit: both tile heights, both forms, both modes)."""
    eng = _engine(name, 3, precision)
    try:
        for which in pf.IMAGES:
            px = pf.image(which, 3)
            x = oracle.img_to_data(px)
            o32, o64 = pf.truth(name, 3, which)
            outs, outs8 = {}, {}
            for cell in CELLS:
                _reset(eng)
                eng.set_pipeline(False)
                for k, v in FORMS[cell].items():
                    eng.set_experiment(k, v)
                outs[cell] = eng.upscale_f32(x)
                _expect_cell(eng, cell, 3, precision, "f32", "f32", 3)
                _check_output(outs[cell], o32, o64, f"{name} {precision} {which} {cell}")
                outs8[cell] = eng.upscale_rgba8(px)
                _expect_cell(eng, cell, 3, precision, "u8", "u8", 3)
                np.testing.assert_array_equal(outs8[cell], _quantise(outs[cell]))
            for cell in CELLS:
                np.testing.assert_array_equal(outs[cell], outs["pipe/8"], err_msg=f"{name} {precision} {which} {cell}")
    finally:
        eng.close()


# ---- (d) the gradient -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pf.GRAD_CASES, ids=pf.grad_case_id)
def test_gradient_against_the_restatement(case):
    name, f, kind, n, h, w, linear = case
    p = pf.weights(name, f)
    hr = pf.grad_case_batch(case)
    eng = _engine(name, f, "f32")   # the inference weights are the family's too: validation_error scores them
    try:
        err, ne, g = eng.backprop(hr, p, linear_loss=linear)
        assert ne == n * 3 * f * (h // f) * f * (w // f)
        lr, _ = gpu_pool(eng, hr)
        _, ne_ref, want = grad_ref.backprop(p, hr, f, linear, None, 0.0, x=lr.astype(np.float64))
        assert ne_ref == ne and np.isfinite(g).all()
        assert_grad_close(g, want, f, pf.grad_case_id(case))
        val = validation_err(eng, hr, linear)
        assert abs(err - val) <= 1e-6 * val, (err, val)
        if name == "init":   # exact zero biases, betas of exactly 0 and 1: their gradient is as alive as any
            for seg in pf.BIASES + pf.BETAS:
                off, m, _ = grad_ref.segments(f)[seg]
                assert np.isfinite(g[off:off + m]).all() and np.abs(g[off:off + m]).max() > 0, seg
    finally:
        eng.close()


# ---- (e) sr_set_params across scales ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_set_params_leaves_nothing_behind_from_the_previous_scale(precision):
    x = oracle.img_to_data(pf.image("synth", 3))
    fresh = {}
    for name in ("imagenet", "tiny", "wide"):
        e = _engine(name, 3, precision)
        try:
            fresh[name] = e.upscale_f32(x)
        finally:
            e.close()
    assert not np.array_equal(fresh["tiny"], fresh["imagenet"]) and not np.array_equal(fresh["wide"], fresh["imagenet"])
    eng = _engine("imagenet", 3, precision)
    try:
        np.testing.assert_array_equal(eng.upscale_f32(x), fresh["imagenet"])
        for name in ("tiny", "imagenet", "wide", "tiny", "imagenet"):
            eng.set_params(pf.weights(name, 3))
            np.testing.assert_array_equal(eng.upscale_f32(x), fresh[name], err_msg=f"after set_params({name})")
            if precision == "split_f16":
                eng.check_domain()
    finally:
        eng.close()
