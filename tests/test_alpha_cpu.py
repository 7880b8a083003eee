"""The transparency path without a GPU: the numpy restatement (tests/alpha_ref.py) against torch's bilinear interpolation and against the
properties include/srhip.h states, the header and the library's exports, and the CLI's argument rules."""
import os
import subprocess

import numpy as np
import pytest

import alpha_ref

ENTRY_POINTS = ("sr_bleed_rgba8_dev", "sr_merge_alpha_rgba8_dev", "sr_upscale_rgba8_alpha_dev", "sr_upscale_rgba8_alpha")
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 9), (37, 129)]


@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_alpha_upscale_is_bilinear_rounded_half_up(f, shape):
    """S / 4 f^2 is torch's half-pixel, edge-clamped bilinear value in f64 (to its rounding error); the byte is within half a step of it."""
    import torch
    a = np.random.default_rng(f * 1000 + shape[0] * shape[1]).integers(0, 256, shape, dtype=np.uint8)
    ref = torch.nn.functional.interpolate(torch.from_numpy(a.astype(np.float64))[None, None], scale_factor=f, mode="bilinear",
                                          align_corners=False)[0, 0].numpy()
    exact = alpha_ref.up_alpha_sum(a, f) / (4.0 * f * f)
    assert exact.shape == ref.shape == (f * shape[0], f * shape[1])
    # torch forms a source coordinate (o + 0.5) / f - 0.5 in f64: at a coordinate near 129 one ulp is 2.8e-14, a few of them land in each
    # axis's weight, and a weight error counts up to 255 times: 1e-10 bounds that with room; a wrong tap or weight is off by 1 / 4 f^2 or more
    assert np.abs(exact - ref).max() <= 1e-10
    out = alpha_ref.up_alpha(a, f)
    assert out.dtype == np.uint8
    assert np.abs(out.astype(np.float64) - ref).max() <= 0.5 + 1e-9
    np.testing.assert_array_equal(out, np.floor(exact + 0.5).astype(np.uint8))


@pytest.mark.parametrize("f", [2, 3, 4])
def test_constant_alpha_stays_constant(f):
    for value in (0, 1, 127, 254, 255):
        for shape in SHAPES:
            assert (alpha_ref.up_alpha(np.full(shape, value, np.uint8), f) == value).all()


@pytest.mark.parametrize("pattern", ["sparse", "dense", "corner", "hole"])
def test_bleed_commutes_with_the_eight_transforms(pattern):
    px = alpha_ref.alpha_pattern(pattern, 13, 21, 3, seed=5)
    for radius in (1, 3, 16):
        ref = alpha_ref.bleed(px, radius)
        for k in range(8):
            np.testing.assert_array_equal(alpha_ref.bleed(alpha_ref.transform(px, k), radius), alpha_ref.transform(ref, k))


@pytest.mark.parametrize("pattern", ["sparse", "dense", "opaque", "transparent", "corner", "hole"])
def test_bleed_leaves_visible_pixels_and_alpha_alone(pattern):
    px = alpha_ref.alpha_pattern(pattern, 23, 17, 4, seed=9)
    np.testing.assert_array_equal(alpha_ref.bleed(px, 0), px)
    for radius in (1, 4, 16):
        out = alpha_ref.bleed(px, radius)
        np.testing.assert_array_equal(out[..., 3], px[..., 3])
        visible = px[..., 3] > 0
        np.testing.assert_array_equal(out[visible], px[visible])
        if pattern in ("opaque", "transparent"):
            np.testing.assert_array_equal(out, px)
    # one step is the rounded mean of the visible neighbours, written out for one pixel
    px = np.zeros((3, 3, 4), np.uint8)
    px[0, 0] = (10, 20, 31, 255)
    px[2, 1] = (11, 21, 30, 1)
    px[0, 2] = (12, 20, 30, 9)
    assert tuple(alpha_ref.bleed(px, 1)[1, 1]) == (11, 20, 30, 0)  # (33 / 3, 61 / 3 = 20.33, 91 / 3 = 30.33)
    px[0, 2] = (13, 20, 30, 0)
    assert tuple(alpha_ref.bleed(px, 1)[1, 1]) == (11, 21, 31, 0)  # (21 / 2 = 10.5 -> 11, 41 / 2 -> 21, 61 / 2 -> 31): halves go up


def test_bleed_of_the_constant_sprite():
    colour = (200, 120, 40)
    px, dist = alpha_ref.disc_sprite(colour)
    out = alpha_ref.bleed(px, 8)
    assert (out[dist <= 7][:, :3] == colour).all()
    assert (dist <= 7).sum() > (dist == 0).sum()
    assert (out[dist > 8][:, :3] == 0).all() and (dist > 8).any()
    assert (out[..., 3] == px[..., 3]).all()


def test_mean_by_multiplication_is_exact():
    """The bleed kernel divides by 2 n with one multiplication (sr_alpha.hip mean_round): exact for every numerator it can meet."""
    for n in range(1, 9):
        recip = -(-(1 << 19) // n)
        num = np.arange(0, 2 * 255 * n + n + 1, dtype=np.uint64)
        assert (num.max() * recip) < (1 << 32)
        np.testing.assert_array_equal((num * recip) >> 20, num // (2 * n))


def test_entry_points_are_declared_and_exported():
    from conftest import ROOT
    from rusty_sr_amd import _lib
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert "#define SR_ALPHA_BLEED_DEFAULT 8" in header and "#define SR_ALPHA_BLEED_MAX 16" in header
    assert f"#define SR_ALPHA_BLEED_TILE {_lib.SR_ALPHA_BLEED_TILE}" in header
    assert (_lib.SR_ALPHA_BLEED_DEFAULT, _lib.SR_ALPHA_BLEED_MAX) == (8, 16) and _lib.SR_ALPHA_BLEED_DEFAULT >= _lib.SR_HALO


def _cli(*args):
    from rusty_sr_amd.build import build_host
    exe = build_host()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # argument errors come before any device is touched
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args,why", [
    (("in.png", "out.png", "--alpha", "-d"), "The argument '--alpha' cannot be used with '--downsample'"),
    (("in.png", "out.png", "--alpha", "--devices", "0,1"), "The argument '--alpha' cannot be used with more than one device"),
    (("in.png", "out.png", "--bleed", "4"), "The following required arguments were not provided:\n    --alpha"),
    (("in.png", "out.png", "--alpha", "--bleed", "17"), "'17' isn't a valid value for '--bleed <N>'"),
    (("in.png", "out.png", "--alpha", "--bleed", "-1"), "'-1' isn't a valid value for '--bleed <N>'"),
    (("in.png", "out.png", "--alpha", "--bleed", "x"), "'x' isn't a valid value for '--bleed <N>'"),
    (("in.png", "out.jpg", "--alpha"), "carry no alpha"),
    (("in.png", "out.bmp", "--alpha", "--bleed", "0"), "carry no alpha"),
])
def test_cli_refuses_bad_alpha_arguments(args, why):
    res = _cli(*args)
    assert res.returncode == 2
    assert why in res.stderr and "USAGE" in res.stderr and res.stderr.endswith("For more information try --help\n"), res.stderr
    assert not os.path.exists(args[1])


def test_cli_help_names_the_options():
    out = _cli("--help").stdout
    assert "--alpha" in out and "--bleed <N>" in out
    for kept in ("--downsample", "--ensemble <N>", "--precision <MODE>", "--devices <N,N,...>", "--timing", "<INPUT_FILE>", "validate"):
        assert kept in out, kept
