"""The metrics' restatement (tests/metrics_ref.py) against independent evaluations, the aggregate's rules, the constants of the binding
and the CLI's usage errors -- nothing here needs a GPU; tests/test_gpu_metrics.py holds the library to the restatement."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import metrics_ref as ref
from conftest import ROOT, synth_u8

CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


def noisy(img, seed, amp=6):
    rng = np.random.default_rng(seed)
    return np.clip(img.astype(np.int32) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w,seed", [(11, 11, 1), (23, 40, 2), (37, 19, 3)])
def test_separable_map_is_the_2d_gaussian_window(h, w, seed):
    """rows-then-columns in f64 against scipy's direct 2-D correlation with outer(g, g), 'valid' positions, per map value."""
    from scipy.signal import correlate2d
    a = synth_u8(seed, 1, h, w)[0]
    b = noisy(a, seed + 10)
    ya, yb = ref.luma(a).astype(np.float64), ref.luma(b).astype(np.float64)
    g = ref.weights()
    assert abs(g.sum() - 1) < 1e-15 and g[5] == g.max() and np.allclose(g, g[::-1], rtol=0, atol=0)
    win = np.outer(g, g)

    def f2(x):
        return correlate2d(x, win, mode="valid")
    ma, mb = f2(ya), f2(yb)
    va, vb, cov = f2(ya * ya) - ma * ma, f2(yb * yb) - mb * mb, f2(ya * yb) - ma * mb
    want = ((2 * ma * mb + ref.C1) * (2 * cov + ref.C2)) / ((ma * ma + mb * mb + ref.C1) * (va + vb + ref.C2))
    got = ref.ssim_map(ref.luma(a), ref.luma(b))
    assert got.shape == want.shape == (h - 10, w - 10)
    assert np.abs(got - want).max() <= 1e-11
    assert np.all(got <= 1 + 1e-12) and got.min() > 0


def test_identical_images_score_exactly_one():
    a = synth_u8(7, 1, 40, 33)[0]
    m = ref.metrics(a, a.copy(), 3)
    assert m["y_sq_err"] == 0 and m["y_psnr"] == math.inf
    assert m["ssim_count"] == (40 - 6 - 10) * (33 - 6 - 10) and m["ssim_sum"] == m["ssim_count"] and m["ssim"] == 1.0
    flat = np.full((20, 20, 3), 255, np.uint8)  # the cancellation case: E[x^2] - mu^2 at 235^2
    assert ref.metrics(flat, flat, 0)["ssim"] == 1.0


def test_luma_is_the_rounded_rational_on_every_colour():
    """(65481 R + 128553 G + 24966 B + 127500) div 255000 + 16 is round-half-up of 16 + (65.481 R + 128.553 G + 24.966 B) / 255 on all 2^24
    colours; 194 of them are exact ties, which the formula takes upward; the double-precision formula misses 39 colours."""
    r, g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    px = np.stack([r, g, b], axis=-1).reshape(-1, 3).astype(np.uint8)
    y = ref.luma(px)
    num = 65481 * r.ravel() + 128553 * g.ravel() + 24966 * b.ravel()   # x 1000 x 255: the exact value is 16 + num / 255000
    rem = num % 255000
    want = 16 + num // 255000 + (2 * rem >= 255000)                     # round to nearest, ties upward, in integers
    assert np.array_equal(y, want)
    ties = np.flatnonzero(2 * rem == 255000)
    assert ties.size == 194
    assert np.array_equal(y[ties], 16 + num[ties] // 255000 + 1)
    assert y.min() == 16 and y.max() == 235
    assert (y[0], y[-1]) == (16, 235)
    for i in (0, 12345, 2 ** 24 - 1, int(ties[0]), int(ties[-1])):     # ... and the same through exact rationals, on a few
        exact = 16 + Fraction(int(num[i]), 255000)
        assert int(y[i]) == math.floor(exact + Fraction(1, 2))
    p = px.astype(np.float64)
    double = np.floor(16 + (65.481 * p[:, 0] + 128.553 * p[:, 1] + 24.966 * p[:, 2]) / 255 + 0.5)  # (the coefficients are no doubles)
    assert np.count_nonzero(double != y) == 39


@pytest.mark.parametrize("h,w,s,y_count,ssim_count", [
    (11, 11, 0, 121, 1), (10, 40, 0, 400, 0), (40, 10, 0, 400, 0), (17, 30, 3, 11 * 24, 1 * 14), (18, 30, 4, 10 * 22, 0),
    (6, 30, 3, 0, 0), (7, 7, 3, 1, 0), (5, 30, 3, 0, 0), (30, 31, 10, 110, 0), (31, 31, 10, 121, 1)])
def test_counts_at_degenerate_sizes(h, w, s, y_count, ssim_count):
    a = synth_u8(h * w, 1, h, w)[0]
    m = ref.metrics(a, noisy(a, 5), s)
    assert (m["y_count"], m["ssim_count"]) == (y_count, ssim_count)
    if ssim_count == 0:
        assert m["ssim_sum"] == 0.0 and m["ssim"] is None
    if y_count == 0:
        assert m["y_sq_err"] == 0 and m["y_psnr"] is None
    with pytest.raises(ValueError):
        ref.metrics(a, a, -1)


def test_binding_helpers_agree_with_the_restatement():
    """The Python side's own arithmetic (y_psnr, ssim_mean, metrics_from_bytes, aggregate_metrics) -- no library call."""
    import struct
    import rusty_sr_amd as r
    a = synth_u8(3, 1, 30, 26)[0]
    b = noisy(a, 4)
    for s in (0, 2, 8, 13):
        want = ref.metrics(a, b, s)
        got = r.metrics_from_bytes(struct.pack("<Qd", want["y_sq_err"], want["ssim_sum"]), 30, 26, s)
        assert got == want
    assert r.y_psnr(0, 5) == math.inf and r.y_psnr(0, 0) is None and r.ssim_mean(0.0, 0) is None
    assert r.y_psnr(65025 * 4, 4) == 0.0


def test_aggregate_skips_and_infinities():
    import rusty_sr_amd as r
    imgs = [
        {"err_sum": 2.0, "n_elems": 300, "y_psnr": 30.0, "ssim": 0.9},
        {"err_sum": 1.0, "n_elems": 100, "y_psnr": 34.0, "ssim": None},    # too small for a window
        {"err_sum": 0.5, "n_elems": 12, "y_psnr": None, "ssim": None},     # nothing left after the shave
        {"err_sum": 0.25, "n_elems": 200, "y_psnr": 35.0, "ssim": 0.8},
    ]
    for agg in (r.aggregate_metrics(imgs), ref.aggregate(imgs)):
        assert agg["skipped"] == [(1, "ssim"), (2, "y_psnr"), (2, "ssim")]
        assert agg["y_psnr"] == pytest.approx(33.0, abs=1e-12) and agg["ssim"] == pytest.approx(0.85, abs=1e-15)
        assert agg["psnr"] == pytest.approx(-10 * math.log10(3.75 / 612), abs=1e-12)
    imgs[0]["y_psnr"] = math.inf  # a zero-error image contributes inf
    assert r.aggregate_metrics(imgs)["y_psnr"] == math.inf == ref.aggregate(imgs)["y_psnr"]
    none = [{"err_sum": 0.0, "n_elems": 3, "y_psnr": None, "ssim": None}]
    agg = r.aggregate_metrics(none)
    assert agg["psnr"] == math.inf and agg["y_psnr"] is None and agg["ssim"] is None and len(agg["skipped"]) == 2


def test_tile_constant_matches_the_header():
    from rusty_sr_amd import _lib
    src = open(os.path.join(ROOT, "include", "srhip.h")).read()
    assert int(re.search(r"#define SR_METRICS_TILE (\d+)", src).group(1)) == _lib.SR_METRICS_TILE
    import ctypes as C
    assert C.sizeof(_lib.Metrics) == 32


def _run(*args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=120)


def test_cli_usage_errors(tmp_path):
    """clap's wording, exit 2, nothing on stdout -- all before any device is touched."""
    d = str(tmp_path)
    cases = [
        (("validate", "--shave", "3", d), "The following required arguments were not provided:\n    --metrics"),
        (("validate", "--metrics", "--shave", "2.5", d), "'2.5' isn't a valid value for '--shave <N>'"),
        (("validate", "--metrics", "--shave", "x", d), "'x' isn't a valid value for '--shave <N>'"),
        (("validate", "--metrics", "--shave", "-1", d), "'-1' isn't a valid value for '--shave <N>'"),
        (("validate", "--metrics", "--shave=", d), "'' isn't a valid value for '--shave <N>'"),
        (("validate", "--metrics", d, "--shave"), "The argument '--shave <N>' requires a value but none was supplied"),
        (("--metrics", "in.png", "out.png"), "The argument '--metrics' can only be used with the 'validate' subcommand"),
        (("--shave", "2", "in.png", "out.png"), "The argument '--shave' can only be used with the 'validate' subcommand"),
        (("train", "--metrics", "p.rsr", d), "The argument '--metrics' can only be used with the 'validate' subcommand"),
    ]
    for args, text in cases:
        res = _run(*args)
        assert res.returncode == 2, (args, res)
        assert res.stdout == "" and res.stderr.startswith("error: " + text + "\n\nUSAGE:\n"), (args, res.stderr)
        assert res.stderr.endswith("For more information try --help\n")


def test_cli_help_names_the_options():
    res = _run("validate", "--help")
    assert res.returncode == 0 and "--metrics " in res.stdout and "--shave <N>" in res.stdout
    rs = open(os.path.join(ROOT, "rust_host", "src", "main.rs")).read()
    cpp = open(os.path.join(ROOT, "rusty_sr_amd", "host", "main.cpp")).read()
    for text in ('"--metrics"', '"--shave"', "Y-PSNR:\\t", "SSIM:\\t", "isn't a valid value for '--shave <N>'",
                 "can only be used with the 'validate' subcommand"):
        assert text in rs and text in cpp, text
