"""Resampling to any size without a GPU: the numpy restatement (tests/resize_ref.py) against Pillow's mode-F Image.resize and against the
two parameter-free graphs of the oracle, the header and the library's exports, and the CLI's argument rules."""
import os
import subprocess

import numpy as np
import pytest

import oracle
import resize_ref

ENTRY_POINTS = ("sr_resize_dev", "sr_resize_rgba8", "sr_upscale_rgba8_sized_dev", "sr_upscale_rgba8_sized")
PILLOW_SHAPES = [((7, 9), (3, 4)), ((5, 31), (8, 50)), ((33, 17), (33, 17)), ((20, 30), (7, 11)), ((1, 1), (4, 5)), ((64, 48), (43, 37)),
                 ((3, 100), (9, 33)), ((12, 12), (36, 36)), ((36, 36), (12, 12))]


@pytest.mark.parametrize("name", resize_ref.FILTERS)
@pytest.mark.parametrize("shape,size", PILLOW_SHAPES)
def test_restatement_is_pillows_resize(name, shape, size):
    """Pillow computes its weights in f64 and stores f32 samples after either pass: 1e-6 is an order above the 1.1e-7 such storing costs on
    values in [0, 1]; a wrong tap or weight is off by far more."""
    from PIL import Image
    pil = {"box": Image.BOX, "triangle": Image.BILINEAR, "catrom": Image.BICUBIC, "lanczos3": Image.LANCZOS}[name]
    x = np.random.default_rng(shape[0] * 1000 + shape[1]).random(shape).astype(np.float32)
    want = np.asarray(Image.fromarray(x, mode="F").resize((size[1], size[0]), pil), dtype=np.float64)
    got = resize_ref.resize_plane(x, size, name)
    assert got.shape == want.shape == size
    assert np.abs(got - want).max() < 1e-6


@pytest.mark.parametrize("shape", [(3, 3), (6, 9), (12, 27)])
def test_box_to_a_third_is_the_downsample_graph(shape):
    x = np.random.default_rng(shape[1]).random((2,) + shape + (3,))
    want = oracle.downsample(x, f64=True)
    got = resize_ref.resize(x, (shape[0] // 3, shape[1] // 3), "box")
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-9


@pytest.mark.parametrize("shape", [(1, 1), (1, 4), (5, 2), (7, 9)])
def test_triangle_to_three_times_is_the_bilinear_graph(shape):
    """... edges included: a two-tap edge clipped to its one tap and renormalised is the clamped edge."""
    x = np.random.default_rng(shape[0] * 31 + shape[1]).random((2,) + shape + (3,))
    want = oracle.bilinear(x, f64=True)
    got = resize_ref.resize(x, (3 * shape[0], 3 * shape[1]), "triangle")
    assert got.shape == want.shape
    assert np.abs(got - want).max() < 1e-9


def test_weights_sum_to_one_and_identity_size_is_the_identity():
    for name in resize_ref.FILTERS:
        for n_in, n_out in ((1, 1), (1, 5), (64, 3), (3, 64), (9, 257), (130, 43)):
            for lo, w in resize_ref.taps(n_in, n_out, name):
                assert 0 <= lo and lo + len(w) <= n_in and len(w) >= 1
                assert abs(w.sum() - 1.0) < 1e-12
        x = np.random.default_rng(3).random((5, 7, 3))
        assert np.abs(resize_ref.resize(x, (5, 7), name, srgb_space=True) - x).max() < 1e-15


def test_scale_rounding_rule():
    """--scale S: max(1, floor(in S + 0.5)) per axis, relative to the INPUT image."""
    assert resize_ref.scaled_size(5, 7, 0.5) == (3, 4)      # halves of odd sizes go up
    assert resize_ref.scaled_size(333, 500, 1.5) == (500, 750)
    assert resize_ref.scaled_size(9, 11, 1.5) == (14, 17)   # 13.5 -> 14, 16.5 -> 17
    assert resize_ref.scaled_size(40, 70, 2) == (80, 140)
    assert resize_ref.scaled_size(1, 3, 0.1) == (1, 1)      # never below one pixel


def test_entry_points_are_declared_and_exported():
    from conftest import ROOT
    from rusty_sr_amd import _lib
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert "enum sr_filter { SR_FILTER_BOX = 0, SR_FILTER_TRIANGLE = 1, SR_FILTER_CATROM = 2, SR_FILTER_LANCZOS3 = 3 };" in header
    assert "enum sr_pixels { SR_PIXELS_RGBA8 = 0, SR_PIXELS_F32 = 1 };" in header and "#define SR_RESIZE_SRGB_SPACE 1" in header
    assert (_lib.SR_FILTER_BOX, _lib.SR_FILTER_TRIANGLE, _lib.SR_FILTER_CATROM, _lib.SR_FILTER_LANCZOS3) == (0, 1, 2, 3)
    assert (_lib.SR_PIXELS_RGBA8, _lib.SR_PIXELS_F32, _lib.SR_RESIZE_SRGB_SPACE) == (0, 1, 1)


def _cli(*args):
    from rusty_sr_amd.build import build_host
    exe = build_host()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # argument errors come before any device is touched
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60)


def _butterfly():
    from conftest import ROOT
    return os.path.join(ROOT, "tests", "golden", "butterfly_lr.png")


@pytest.mark.parametrize("args,why", [
    (("in.png", "out.png", "--size", "640x480", "--scale", "2"), "The argument '--size <WxH>' cannot be used with '--scale <S>'"),
    (("in.png", "out.png", "--filter", "box"), "The following required arguments were not provided:\n    <--size <WxH>|--scale <S>>"),
    (("in.png", "out.png", "--resize-space", "srgb"), "The following required arguments were not provided:\n    <--size <WxH>|--scale <S>>"),
    (("in.png", "out.png", "--size", "640x480", "-d"), "The argument '--size <WxH>' cannot be used with '--downsample'"),
    (("in.png", "out.png", "--scale", "1.5", "--downsample"), "The argument '--scale <S>' cannot be used with '--downsample'"),
    (("in.png", "out.png", "--size", "640x480", "--alpha"), "The argument '--size <WxH>' cannot be used with '--alpha'"),
    (("in.png", "out.png", "--scale", "2", "--alpha"), "The argument '--scale <S>' cannot be used with '--alpha'"),
    (("in.png", "out.png", "--size", "640x480", "--devices", "0,1"), "The argument '--size <WxH>' cannot be used with more than one device"),
    (("in.png", "out.png", "--scale", "2", "--devices", "0,1"), "The argument '--scale <S>' cannot be used with more than one device"),
    (("in.png", "out.png", "--size", "640"), "'640' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "640x"), "'640x' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "0x480"), "'0x480' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "-4x480"), "'-4x480' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "16385x480"), "'16385x480' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "640x16385"), "'640x16385' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--size", "6.5x4"), "'6.5x4' isn't a valid value for '--size <WxH>'"),
    (("in.png", "out.png", "--scale", "0"), "'0' isn't a valid value for '--scale <S>'"),
    (("in.png", "out.png", "--scale", "-1"), "'-1' isn't a valid value for '--scale <S>'"),
    (("in.png", "out.png", "--scale", "x"), "'x' isn't a valid value for '--scale <S>'"),
    (("in.png", "out.png", "--scale", "1e3"), "'1e3' isn't a valid value for '--scale <S>'"),
    (("in.png", "out.png", "--scale", "1.5.2"), "'1.5.2' isn't a valid value for '--scale <S>'"),
    (("in.png", "out.png", "--size", "64x48", "--filter", "cubic"), "'cubic' isn't a valid value for '--filter <FILTER>'"),
    (("in.png", "out.png", "--size", "64x48", "--resize-space", "gamma"), "'gamma' isn't a valid value for '--resize-space <SPACE>'"),
    (("in.png", "out.png", "--size"), "The argument '--size <WxH>' requires a value but none was supplied"),
])
def test_cli_refuses_bad_resize_arguments(args, why):
    res = _cli(*args)
    assert res.returncode == 2
    assert why in res.stderr and "USAGE" in res.stderr and res.stderr.endswith("For more information try --help\n"), res.stderr
    assert not os.path.exists(args[1])


def test_cli_refuses_a_scale_that_exceeds_the_largest_output(tmp_path):
    """The input's header says how large it is: refused before any device is touched (butterfly_lr.png is 167 pixels wide)."""
    out = str(tmp_path / "out.png")
    res = _cli(_butterfly(), out, "--scale", "100")
    assert res.returncode == 2
    assert "'100' isn't a valid value for '--scale <S>'" in res.stderr and "USAGE" in res.stderr, res.stderr
    assert not os.path.exists(out)


@pytest.mark.parametrize("args", [
    ("--size", "500x333"), ("--scale", "1.5", "--filter", "catrom"), ("--scale=0.5", "--resize-space=srgb", "-p", "bilinear"),
    ("--size=64x48", "--filter=box", "--ensemble", "8", "--precision", "split_f16", "--timing"),
    ("--size", "64X48", "-c", "weights.rsr"),
])
def test_cli_accepts_the_combinations(args, tmp_path):
    """The size options combine with -p (bilinear included), -c, --ensemble, --precision and --timing: such a command line passes the
    argument rules and fails only for want of a device (or of the custom parameter file), never with a usage error."""
    res = _cli(_butterfly(), str(tmp_path / "out.png"), *args)
    assert res.returncode != 0 and res.returncode != 2, res.stderr
    assert "USAGE" not in res.stderr, res.stderr


def test_cli_help_names_the_options():
    out = _cli("--help").stdout
    for new in ("--size <WxH>", "--scale <S>", "--filter <FILTER>", "--resize-space <SPACE>", "box, triangle, catrom", "lanczos3", "linear, srgb"):
        assert new in out, new
    for kept in ("--downsample", "--ensemble <N>", "--precision <MODE>", "--devices <N,N,...>", "--timing", "--alpha", "--bleed <N>",
                 "<INPUT_FILE>", "validate"):
        assert kept in out, kept
