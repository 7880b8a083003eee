"""What every synchronous host-pointer call beside the plain upscale owes its caller (include/srhip.h sr_set_precision, sr_check_domain,
sr_last_timing), checked through the ensemble, validation and transparency calls themselves: in the split-half mode a value that leaves
the domain makes the call run again in exact f32 and the mode is switched back; a fault an earlier *_dev call left is set aside, not
taken for the call's own; with profiling on the call's times are there to read.  Images are 40 x 72 LR (120 x 216 HR), the bundled
`imagenet` parameters, factor 3."""
import numpy as np
import pytest

from conftest import synth_u8

pytestmark = pytest.mark.gpu

LH, LW, F = 40, 72, 3
MASK = 0b10011  # members 0, 1 and the axis-swapping member 4


def engine(p, precision):
    import rusty_sr_amd as r
    return r.Engine(p, device=0, precision=precision)


def poisoned(x):
    y = x.copy()
    y[20, 30, 1] = 1e6
    return y


def test_f32_calls_fall_back_to_exact_f32_and_switch_back(params):
    p = params["imagenet"]
    rng = np.random.default_rng(21)
    lr = rng.random((LH, LW, 3), dtype=np.float32)
    hr = rng.random((F * LH, F * LW, 3), dtype=np.float32)
    calls = {
        "ensemble": (lambda e, bad: e.upscale_ensemble_f32(poisoned(lr) if bad else lr, MASK), np.array_equal),
        "validation": (lambda e, bad: e.validation_error(poisoned(hr) if bad else hr), lambda a, b: a == b),
        "validation_pair": (lambda e, bad: e.validation_error_pair(poisoned(lr) if bad else lr, hr), lambda a, b: a == b),
    }
    split, f32, fresh = engine(p, "split_f16"), engine(p, "f32"), engine(p, "split_f16")
    assert not np.array_equal(fresh.upscale_ensemble_f32(lr, MASK), f32.upscale_ensemble_f32(lr, MASK))  # the modes differ in the last bits
    for name, (call, same) in calls.items():
        got, want = call(split, True), call(f32, True)
        assert same(got, want), name  # bit for bit: only a recompute in exact f32 gives that
        split.check_domain()  # the synchronous call has dealt with it
        assert same(call(split, False), call(fresh, False)), name  # the mode was switched back
    for e in (split, f32, fresh):
        e.close()


def test_u8_calls_fall_back_to_exact_f32(params):
    p = params["imagenet"].copy()
    p[2400:2432] = 7e4  # f_bias: every input value is small, the first layer's outputs are not
    rgba = np.empty((LH, LW, 4), dtype=np.uint8)
    rgba[..., :3] = synth_u8(22, 1, LH, LW)[0]
    rgba[..., 3] = 255
    rgba[:, LW // 2:, 3] = 0  # half transparent
    hr = synth_u8(23, 1, F * LH, F * LW)[0]
    split, f32 = engine(p, "split_f16"), engine(p, "f32")
    np.testing.assert_array_equal(split.upscale_rgba8_alpha(rgba), f32.upscale_rgba8_alpha(rgba))
    split.check_domain()
    np.testing.assert_equal(split.validation_metrics(hr), f32.validation_metrics(hr))  # the loss and the scores (NaN, were there one, as itself)
    split.check_domain()
    split.close()
    f32.close()


def test_a_stale_device_fault_is_set_aside_by_every_host_call(params):
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    p = params["imagenet"]
    x = np.random.default_rng(24).random((1, LH, LW, 3), dtype=np.float32)
    bad = x.copy()
    bad[0, 20, 30, 1] = 1e6
    px = synth_u8(25, 1, LH, LW)[0]
    rgba = np.dstack([px, np.full((LH, LW, 1), 200, dtype=np.uint8)])
    hr = synth_u8(26, 1, F * LH, F * LW)[0]
    calls = {
        "ensemble": (lambda e: e.upscale_ensemble_f32(x[0], MASK), np.array_equal),
        "validation": (lambda e: e.validation_error(hr), lambda a, b: a == b),
        "alpha": (lambda e: e.upscale_rgba8_alpha(rgba), np.array_equal),
    }
    fresh = engine(p, "split_f16")
    want = {name: call(fresh) for name, (call, _) in calls.items()}
    fresh.close()
    eng = engine(p, "split_f16")
    for name, (call, same) in calls.items():
        eng.upscale_f32_dev(torch.from_numpy(bad).cuda())  # leaves a fault nobody has checked for
        torch.cuda.synchronize()
        assert same(call(eng), want[name]), name  # the split-half mode's bits: the fault was not taken for this call's
        with pytest.raises(r.SrError) as e:
            eng.check_domain()
        assert e.value.status == _lib.SR_E_DOMAIN
        eng.check_domain()  # reported once
    eng.close()


def test_profiled_host_calls_report_their_times(params):
    """Each call on an engine of its own, whose times are all 0 before it."""
    px = synth_u8(27, 1, LH, LW)[0]
    rgba = np.dstack([px, np.full((LH, LW, 1), 200, dtype=np.uint8)])
    hr = synth_u8(28, 1, F * LH, F * LW)[0]
    calls = {
        "ensemble": (lambda e: e.upscale_ensemble_rgba8(px, MASK), ("h2d_ms", "total_ms", "d2h_ms")),
        "alpha": (lambda e: e.upscale_rgba8_alpha(rgba), ("h2d_ms", "total_ms", "d2h_ms")),
        "validation": (lambda e: e.validation_error(hr), ("total_ms",)),
    }
    for name, (call, keys) in calls.items():
        eng = engine(params["imagenet"], "f32")
        eng.set_profiling(True)
        assert not any(eng.last_timing()[k] for k in keys)
        call(eng)
        t = eng.last_timing()
        eng.close()
        assert all(t[k] > 0 for k in keys), (name, t)
