"""The parameter families of tests/param_families.py on the CPU oracle alone, without a GPU: the gate of tests/test_gpu_param_families.py.
Each family is seeded, is what it claims to be, and is one on which the reference itself is well conditioned -- so that a failure of
the GPU table is the kernels' and not the reference's.  A family, image or case that fails a gate leaves the GPU table; no bar is
widened for it.

Left out, with the measured values:
  gradient case tiny-f3-u8_3-n2-20x23-mse: the f32 run of the restatement is 4.9e-4 (conv7; conv9 4.0e-4, conv10 3.7e-4) from the f64
      run, against the gate's 1e-5 -- l1..l3 are ~3e-4, where sqrt(z^2 + 1) - 1 cancels in f32;
  gradient case dim-f3-u8_3-n2-20x23-mse: 1.3e-4 (conv1, conv2, conv3) -- the same cancellation in node f, which is ~3e-4.
Nothing else: every family passes the output and node gates at every factor and on both images (the worst |f32 - f64| of the
oracle: 1.6e-6 at the output, `wide` at factors 3 and 4; 1.7e-5 on a node of 17.6, the control row imagenet.rsr on white noise)."""
import hashlib

import numpy as np
import pytest
import torch

import grad_ref
import oracle
import param_families as pf
from test_pixel_classes_cpu import _f32_restatement_gradient

CASES = [(name, f) for name in pf.FAMILIES for f in pf.FACTORS]
ids = lambda c: f"{c[0]}-f{c[1]}"

# bundled_scale(factor, seed) as the four copies it replaced made it (tests/test_gpu_kernel_matrix.py, test_gpu_validation.py,
# test_grad_restatement.py and test_gpu_parity.py before they imported it; compared with np.array_equal then): sha256[:16] of the bytes
BUNDLED_DIGESTS = {(2, 5): "e290c2a794002d97", (2, 77): "4db6e824fa1f15cc", (2, 102): "cd2de4f145969214",
                   (3, 5): "5cd600c1bca43f21", (3, 77): "f6a42372235a694c", (3, 103): "03eb527f9759e090",
                   (4, 5): "11f1b650048ce084", (4, 77): "16f09dfe704b28fd", (4, 104): "f82ba842c9b92731"}


def test_bundled_scale_is_what_the_suite_has_always_fed_the_kernels():
    for (f, seed), want in BUNDLED_DIGESTS.items():
        assert hashlib.sha256(pf.bundled_scale(f, seed).tobytes()).hexdigest()[:16] == want, (f, seed)
    import test_gpu_kernel_matrix, test_gpu_parity, test_gpu_validation, test_grad_restatement
    for fn in (test_gpu_kernel_matrix._synthetic_params, test_gpu_parity._synthetic_params, test_gpu_validation.synthetic_params,
               test_grad_restatement.synthetic_params):
        assert fn is pf.bundled_scale


# ---- seeded ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [("bundled_scale", f) for f in pf.FACTORS], ids=ids)
def test_generators_are_seeded(case):
    name, f = case
    a, b, c = pf.family(name, f, 11), pf.family(name, f, 11), pf.family(name, f, 12)
    assert a.dtype == np.float32 and a.shape == (grad_ref.num_params(f),) and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, c)
    b[:] = 0   # the module's caches hand out copies
    assert np.array_equal(a, pf.family(name, f, 11))


# ---- each family is what it claims to be ----------------------------------------------------------------------------------------------
def _seg(p, f, name):
    off, n, shape = grad_ref.segments(f)[name]
    return p[off:off + n].reshape(shape)


@pytest.mark.parametrize("f", pf.FACTORS)
def test_init_has_exact_zero_biases_and_zero_or_one_betas(f):
    p = pf.weights("init", f)
    for name in pf.BIASES:
        assert (_seg(p, f, name) == 0).all(), name
    for name in pf.BETAS:
        b = _seg(p, f, name)
        assert ((b == 0) | (b == 1)).all() and (b == 0).any() and (b == 1).any(), name
    for name in pf.LATER_CONVS:
        assert 0.004 <= _seg(p, f, name).std() <= 0.009, (name, _seg(p, f, name).std())


@pytest.mark.parametrize("f", pf.FACTORS)
def test_early_has_moved_most_parameters_by_a_step(f):
    moved = float((np.abs(pf.weights("early", f).astype(np.float64) - pf.weights("init", f)) >= 1e-3).mean())
    print(f"early f{f}: {moved:.3f} of the parameters moved by >= 1e-3")   # measured 0.89 / 0.88 / 0.93
    assert moved >= 0.5


@pytest.mark.parametrize("f", pf.FACTORS)
def test_wide_spreads_magnitudes_inside_every_kernel_row(f):
    p = pf.weights("wide", f)
    share = pf.share_below(p, f, pf.LATER_CONVS)
    assert share >= 0.20, share   # measured 0.26 / 0.30 / 0.27
    w = np.abs(_seg(p, f, "conv1").astype(np.float64))
    row = w.reshape(32, 5, 5 * 32)   # a kernel row: the 5 x 32 weights of (output channel, ky)
    assert (row.max(axis=-1) >= 2.0 ** 6 * row.min(axis=-1)).all()
    taps5 = w.transpose(0, 1, 3, 2)   # ... and most single (output channel, ky, input channel) rows of five taps, the Winograd triples' rows
    assert (taps5.max(axis=-1) >= 2.0 ** 6 * taps5.min(axis=-1)).mean() >= 0.5   # measured 0.90 .. 0.93
    for name in pf.BETAS:
        b = _seg(p, f, name)
        assert b.min() >= -2 and b.max() <= 3 and (b < -0.5).any() and (b > 1.5).any(), name
    for name in pf.CONVS:
        assert abs(_seg(p, f, name).std() - 0.03) < 1e-4, name


@pytest.mark.parametrize("f", pf.FACTORS)
def test_tiny_has_most_weights_below_the_smallest_normal_half(f):
    p, base = pf.weights("tiny", f), pf.bundled_scale(f, pf.seed_of(f))
    assert pf.share_below(p, f, pf.LATER_CONVS) >= 0.60   # measured 0.96
    for name in ("conv0",) + pf.BETAS:
        assert np.array_equal(_seg(p, f, name), _seg(base, f, name)), name
    for name in pf.LATER_CONVS + pf.BIASES:
        assert np.array_equal(_seg(p, f, name), _seg(base, f, name) * np.float32(1e-3)), name


@pytest.mark.parametrize("f", pf.FACTORS)
def test_dim_scales_the_first_layer_alone(f):
    p, base = pf.weights("dim", f), pf.bundled_scale(f, pf.seed_of(f))
    for name in grad_ref.segments(f):
        want = _seg(base, f, name) * np.float32(1e-3) if name in ("conv0", "f_bias") else _seg(base, f, name)
        assert np.array_equal(_seg(p, f, name), want), name


@pytest.mark.parametrize("which", pf.IMAGES)
def test_dim_puts_node_f_below_the_smallest_normal_half_and_l1_above(which):
    _, t64, _, _ = pf.taps("dim", which)
    small_f, small_l1 = float((np.abs(t64["f"]) < pf.SMALL).mean()), float((np.abs(t64["l1"]) < pf.SMALL).mean())
    print(f"dim {which}: {small_f:.3f} of f and {small_l1:.4f} of l1 below 2^-14")   # measured 0.69 / 0.63 and 0.00
    assert small_f >= 0.5 and small_l1 < 0.01
    _, t64, _, _ = pf.taps("tiny", which)   # ... and tiny the other way round
    assert (np.abs(t64["f"]) < pf.SMALL).mean() < 0.01 and (np.abs(t64["l1"]) < pf.SMALL).mean() >= 0.5


# ---- the oracle is well conditioned on the family -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", pf.IMAGES)
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_oracle_output_is_well_conditioned_and_the_restatements_agree(case, which):
    name, f = case
    o32, o64 = pf.truth(name, f, which)
    top = float(np.abs(o64).max())
    err = float(np.abs(o32.astype(np.float64) - o64).max())
    assert np.isfinite(o32).all() and np.isfinite(o64).all()
    assert err <= 1e-5 * max(1.0, top), (err, top)
    x = oracle.img_to_data(pf.image(which, f)).astype(np.float64)
    got = grad_ref.forward(torch.from_numpy(pf.weights(name, f).astype(np.float64)), torch.from_numpy(x), f).numpy()
    assert np.abs(got - o64).max() <= 1e-11 * top


@pytest.mark.parametrize("which", pf.IMAGES)
@pytest.mark.parametrize("name", ("imagenet",) + pf.FAMILIES)
def test_oracle_nodes_are_well_conditioned(name, which):
    t32, t64, o32, o64 = pf.taps(name, which)
    line = []
    for k in pf.NODES + ("e",):
        top, err = float(np.abs(t64[k]).max()), float(np.abs(t32[k].astype(np.float64) - t64[k]).max())
        line.append(f"{k} {top:.3g} / {err:.1e}")
        assert np.isfinite(t32[k]).all() and err <= 1e-5 * max(1.0, top), (k, err, top)
    print(f"{name} {which}: node maximum / oracle |f32 - f64|: " + ", ".join(line))
    assert np.abs(o32.astype(np.float64) - o64).max() <= 1e-5 * max(1.0, float(np.abs(o64).max()))
    if name != "imagenet":   # the node image is the first of the output table's batch
        np.testing.assert_array_equal(o64[0], pf.truth(name, 3, which)[1][0])


# ---- gradient cases -------------------------------------------------------------------------------------------------------------------
def _gate(case):
    """worst per-segment |f32 - f64| / |f64| of the restatement's gradient, and whether the case passes the gate of
    tests/test_pixel_classes_cpu.py test_gradient_cases_are_well_conditioned (the same two measures, the same floor)"""
    name, f, kind, n, h, w, linear = case
    hr = pf.grad_case_batch(case)
    p = pf.weights(name, f)
    hr64 = grad_ref.hr_values(hr)
    x, target = grad_ref.pool(hr64, f), grad_ref.crop(hr64, f)
    _, _, want = grad_ref.backprop(p, hr, f, linear, None, 0.0)
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    got = _f32_restatement_gradient(p, x, target, f, linear, 1.0 / target.numel())
    floor = 1e-8 * np.abs(want).max()
    worst, ok = 0.0, True
    for seg, (off, m, _) in grad_ref.segments(f).items():
        d, wseg = got[off:off + m] - want[off:off + m], want[off:off + m]
        if np.linalg.norm(wseg) > 0:
            worst = max(worst, np.linalg.norm(d) / np.linalg.norm(wseg))
        ok = ok and np.linalg.norm(d) <= 1e-5 * np.linalg.norm(wseg) + floor and np.abs(d).max() <= 1e-4 * np.abs(wseg).max() + floor
    return worst, ok, want


@pytest.mark.parametrize("case", pf.GRAD_CASES, ids=pf.grad_case_id)
def test_gradient_cases_are_well_conditioned(case):
    worst, ok, want = _gate(case)
    print(f"gate {pf.grad_case_id(case)}: worst segment |f32 - f64| / |f64| = {worst:.2e}")
    assert ok, worst
    if case[0] == "init":   # exact zero biases and 0 / 1 betas still have a gradient
        for seg in pf.BIASES + pf.BETAS:
            off, m, _ = grad_ref.segments(case[1])[seg]
            assert np.abs(want[off:off + m]).max() > 0, seg


@pytest.mark.parametrize("case", pf.GATED_OUT, ids=pf.grad_case_id)
def test_the_cases_left_out_fail_the_gate(case):
    """tiny 4.9e-4, dim 1.3e-4 (measured): ten times and more beyond the gate, so the 1e-4 bar of assert_grad_close would measure the
    conditioning of the case and not the kernel"""
    worst, ok, _ = _gate(case)
    print(f"gate {pf.grad_case_id(case)}: {worst:.2e}")
    assert not ok and worst > 1e-5


def test_gradient_table_is_the_issues_minus_what_the_gate_refuses():
    assert set(pf.GRAD_CASES) | set(pf.GATED_OUT) == set(pf.ALL_GRAD_CASES) and not set(pf.GRAD_CASES) & set(pf.GATED_OUT)
    assert {c[0] for c in pf.GATED_OUT} == {"tiny", "dim"}
