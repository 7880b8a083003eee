"""The border modes (include/srhip.h "Borders") where no GPU is needed: the premise of the feature on the CPU oracle, the index rule
of rusty_sr_amd/csrc/sr_border.h -- the header the pad kernel compiles -- against np.pad through a plain C++ program, the CLI's argv
surface and the constants."""
import os
import re
import subprocess

import numpy as np
import pytest

import border_ref
import oracle
from conftest import ROOT

ENTRY_POINTS = ("sr_pad_rgba8_dev", "sr_pad_f32_dev", "sr_crop_rgba8_dev", "sr_crop_f32_dev", "sr_upscale_rgba8_border_dev",
                "sr_upscale_f32_border_dev", "sr_upscale_rgba8_border", "sr_upscale_f32_border")
MODE_ID = {"wrap": 1, "replicate": 2, "mirror": 3}


# ---- the premise: with pad >= SR_HALO the cropped result of the padded image is that of the infinitely continued plane

def test_wrap_padding_by_the_halo_is_the_tiled_plane_on_the_oracle(params):
    """oracle.forward, imagenet, a random 23 x 29 image: the centre of the wrap-padded forward equals the centre tile of the 3 x 3 tiling
    bit for bit at p = 7 = SR_HALO and p = 8 = SR_BORDER_PAD_DEFAULT, and does not at p = 6."""
    from rusty_sr_amd import _lib
    h, w, f = 23, 29, 3
    x = np.random.default_rng(2024).random((h, w, 3), dtype=np.float32)
    tiled = oracle.forward(params["imagenet"], np.tile(x, (3, 3, 1)))[0]
    want = tiled[f * h:2 * f * h, f * w:2 * f * w]
    got = {p: border_ref.centre(oracle.forward(params["imagenet"], border_ref.pad(x, "wrap", p))[0], f, p) for p in (6, 7, 8)}
    assert _lib.SR_HALO == 7 and _lib.SR_BORDER_PAD_DEFAULT == 8
    for p in (_lib.SR_HALO, _lib.SR_BORDER_PAD_DEFAULT):
        assert got[p].shape == want.shape
        np.testing.assert_array_equal(got[p].view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got[6], want)   # one pixel short of the receptive field: the seam is back (3.0e-3 at the most here)


# ---- the index rule, host-side, from the kernel's header

SIZES, PADS = (1, 2, 3, 7, 8, 33), (0, 1, 7, 8, 32)


def _build_index_program(tmp_path, sanitize):
    exe = str(tmp_path / ("border_index_san" if sanitize else "border_index"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "border_index.cpp"), "-o", exe])
    return exe


def _triples():
    return [(mode, size, p) for mode in border_ref.MODES for size in SIZES for p in PADS]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_index_rule_is_np_pad(tmp_path, sanitize):
    """Every mode, size and pad in one run of the program (and once more under AddressSanitizer and UBSan: host code with its own main)."""
    exe = _build_index_program(tmp_path, sanitize)
    triples = _triples()
    argv = [str(v) for mode, size, p in triples for v in (MODE_ID[mode], size, p)]
    res = subprocess.run([exe, *argv], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(triples)
    for (mode, size, p), line in zip(triples, lines):
        got = np.array(line.split(), dtype=np.int64)
        want = np.pad(np.arange(size), (p, p), mode=border_ref.NP_MODE[mode])
        np.testing.assert_array_equal(got, want, err_msg=f"{mode} size {size} pad {p}")


def test_index_program_refuses_bad_input(tmp_path):
    exe = _build_index_program(tmp_path, False)
    assert subprocess.run([exe, "4", "3", "1"], capture_output=True).returncode == 2
    assert subprocess.run([exe, "1", "3"], capture_output=True).returncode == 2


def test_ref_is_separable_and_crop_inverts_pad():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (2, 5, 3, 4), dtype=np.uint8)
    for mode in border_ref.MODES:
        for p in (0, 1, 8):
            big = border_ref.pad(img, mode, p)
            assert big.shape == (2, 5 + 2 * p, 3 + 2 * p, 4)
            np.testing.assert_array_equal(border_ref.crop(big, p, p, 5, 3), img)
            iy = np.pad(np.arange(5), (p, p), mode=border_ref.NP_MODE[mode])
            ix = np.pad(np.arange(3), (p, p), mode=border_ref.NP_MODE[mode])
            np.testing.assert_array_equal(big, img[:, iy][:, :, ix])


# ---- the ABI and its constants

def test_entry_points_are_declared_and_exported():
    from rusty_sr_amd import _lib
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert name + "(" in header and hasattr(L, name) and name in _lib.SYMBOLS, name


def test_header_constants_match_binding():
    from rusty_sr_amd import _lib
    from rusty_sr_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "srhip.h")).read()
    rust = open(os.path.join(ROOT, "rust_host", "src", "srhip.rs")).read()
    for name in ("SR_BORDER_WRAP", "SR_BORDER_REPLICATE", "SR_BORDER_MIRROR", "SR_BORDER_PAD_DEFAULT", "SR_BORDER_PAD_MAX"):
        val = int(re.search(r"#define %s (\d+)" % name, header).group(1))
        assert val == getattr(_lib, name), name
        assert f"pub const {name}: c_int = {val};" in rust, name
    assert (_lib.SR_BORDER_WRAP, _lib.SR_BORDER_REPLICATE, _lib.SR_BORDER_MIRROR) == (1, 2, 3)
    assert _lib.SR_HALO <= _lib.SR_BORDER_PAD_DEFAULT <= _lib.SR_BORDER_PAD_MAX == 32
    assert Engine.BORDERS == {"wrap": 1, "replicate": 2, "mirror": 3} and set(Engine.BORDERS) == set(border_ref.MODES)


# ---- the CLI's argv surface

def _cli(*args):
    from rusty_sr_amd.build import build_host
    exe = build_host()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # argument errors come before any device is touched
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args,why", [
    (("in.png", "out.png", "--border", "wrap", "-d"), "The argument '--border <MODE>' cannot be used with '--downsample'"),
    (("in.png", "out.png", "--border", "wrap", "--size", "64x64"), "The argument '--border <MODE>' cannot be used with '--size <WxH>'"),
    (("in.png", "out.png", "--border=mirror", "--scale", "2"), "The argument '--border <MODE>' cannot be used with '--scale <S>'"),
    (("in.png", "out.png", "--border", "wrap", "--devices", "0,1"), "The argument '--border <MODE>' cannot be used with more than one device"),
    (("in.png", "out.png", "--border", "zero"), "'zero' isn't a valid value for '--border <MODE>'"),
    (("in.png", "out.png", "--border", ""), "'' isn't a valid value for '--border <MODE>'"),
    (("in.png", "out.png", "--border", "wrap", "--border-pad", "6"), "'6' isn't a valid value for '--border-pad <N>'"),
    (("in.png", "out.png", "--border", "wrap", "--border-pad", "33"), "'33' isn't a valid value for '--border-pad <N>'"),
    (("in.png", "out.png", "--border", "wrap", "--border-pad=x"), "'x' isn't a valid value for '--border-pad <N>'"),
    (("in.png", "out.png", "--border-pad", "8"), "The following required arguments were not provided:\n    --border <MODE>"),
    (("in.png", "out.png", "--border"), "The argument '--border <MODE>' requires a value but none was supplied"),
])
def test_cli_refuses_bad_border_arguments(args, why):
    res = _cli(*args)
    assert res.returncode == 2
    assert why in res.stderr and "USAGE" in res.stderr and res.stderr.endswith("For more information try --help\n"), res.stderr
    assert not os.path.exists(args[1])


def test_cli_help_names_the_options():
    out = _cli("--help").stdout
    assert "--border <MODE>" in out and "--border-pad <N>" in out and "wrap, replicate, mirror" in out
    for kept in ("--downsample", "--ensemble <N>", "--alpha", "--bleed <N>", "--size <WxH>", "--precision <MODE>", "--timing", "<INPUT_FILE>"):
        assert kept in out, kept
