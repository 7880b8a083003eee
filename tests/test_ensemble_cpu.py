"""The self-ensemble without a GPU: the numpy restatement (tests/ensemble_ref.py) against itself and the CPU oracle, the header and the
library's exports, and the CLI's argument rules."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from conftest import ROOT, synth_u8
from ensemble_ref import T, T_inv, ensemble

ENTRY_POINTS = ("sr_upscale_ensemble_f32_dev", "sr_upscale_ensemble_rgba8_dev", "sr_upscale_ensemble_f32", "sr_upscale_ensemble_rgba8",
                "sr_pool_validation_error_ensemble_rgba8", "sr_pair_validation_error_ensemble_rgba8")

# ensemble(T_j x) and T_j ensemble(x) run the same 8 network passes but add their outputs in another order (member k of T_j x is member
# k' of x): they agree up to f32 summation order only.  The largest deviation seen on the CPU over every j and the shapes and seeds of
# test_ensemble_commutes_with_the_transforms is 1.79e-7 (the test prints it); 4x that for other shapes and seeds.
EQUIVARIANCE_TOL = 4 * 1.79e-7


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 5, 3), (5, 1, 3), (7, 12, 3), (13, 4, 4)])
def test_inverse_undoes_transform(shape):
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    for k in range(8):
        y = T(x, k)
        assert y.shape == ((shape[1], shape[0]) if k & 4 else shape[:2]) + shape[2:]
        np.testing.assert_array_equal(T_inv(y, k), x)
        np.testing.assert_array_equal(T(T_inv(x, k), k), x)


def test_members_are_distinct_and_as_defined():
    x = np.arange(6 * 6 * 3, dtype=np.float32).reshape(6, 6, 3)
    seen = [T(x, k).tobytes() for k in range(8)]
    assert len(set(seen)) == 8
    # the definition, element by element: swap (k & 4), then rows (k & 2), then columns (k & 1)
    x = np.arange(3 * 5 * 2).reshape(3, 5, 2)
    for k in range(8):
        y = T(x, k)
        for i in range(y.shape[0]):
            for j in range(y.shape[1]):
                i1 = y.shape[0] - 1 - i if k & 2 else i
                j1 = y.shape[1] - 1 - j if k & 1 else j
                np.testing.assert_array_equal(y[i, j], x[j1, i1] if k & 4 else x[i1, j1])


def test_accumulation_order_and_mask():
    outs = {k: np.float32(0.1) * np.float32(k + 1) for k in range(8)}

    def fwd(x):  # a "network" that names the member it was given: x is T_k of an image holding k
        return np.full((2, 2, 3), outs[int(x.flat[0])], np.float32)

    for m in (0x03, 0xA5, 0xFF):
        ks = [k for k in range(8) if m >> k & 1]
        # (fwd sees T_k(x); make x constant per call so that the member is recoverable)
        acc = np.float32(0)
        for k in ks:
            acc = np.float32(acc + outs[k])
        want = np.float32(acc * (np.float32(1) / np.float32(len(ks))))
        got = [T_inv(fwd(T(np.full((1, 1, 3), k, np.float32), k)), k) for k in ks]
        from ensemble_ref import accumulate
        assert accumulate(got, len(ks)).dtype == np.float32
        np.testing.assert_array_equal(accumulate(got, len(ks)), np.full((2, 2, 3), want))
    with pytest.raises(ValueError):
        ensemble(fwd, np.zeros((1, 1, 3), np.float32), 0)
    with pytest.raises(ValueError):
        ensemble(fwd, np.zeros((1, 1, 3), np.float32), 256)


def test_ensemble_commutes_with_the_transforms(params, capsys):
    p = params["imagenet"]
    fwd = lambda x: oracle.forward(p, x)[0]
    worst = 0.0
    for seed, (h, w) in enumerate([(9, 14), (16, 16), (5, 23)]):
        x = oracle.img_to_data(synth_u8(400 + seed, 1, h, w))[0]
        base = ensemble(fwd, x, 0xFF)
        assert base.dtype == np.float32 and base.shape == (3 * h, 3 * w, 3)
        for j in range(8):
            worst = max(worst, float(np.abs(ensemble(fwd, T(x, j), 0xFF) - T(base, j)).max()))
    with capsys.disabled():
        print(f"\n[ensemble equivariance] largest deviation {worst:.3e} (bound {EQUIVARIANCE_TOL:.3e})")
    assert worst <= EQUIVARIANCE_TOL


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "srhip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(sr_ctx\* ctx, ", text, re.M), name
    for name, value in (("SR_ENSEMBLE_ALL", "0xFFu"), ("SR_ENSEMBLE_FLIPS", "0x0Fu"), ("SR_ENSEMBLE_HFLIP", "0x03u")):
        assert re.search(r"^#define " + name + r" " + value + r"\b", text, re.M), name
    from rusty_sr_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS
    assert (_lib.SR_ENSEMBLE_ALL, _lib.SR_ENSEMBLE_FLIPS, _lib.SR_ENSEMBLE_HFLIP) == (0xFF, 0x0F, 0x03)


def _cli(*args):
    from rusty_sr_amd.build import build_host
    exe = build_host()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # argument errors come before any device is touched
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60)


@pytest.mark.parametrize("args,why", [
    (("in.png", "out.png", "--ensemble", "3"), "isn't a valid value for '--ensemble <N>'"),
    (("in.png", "out.png", "--ensemble"), "requires a value"),
    (("in.png", "out.png", "--ensemble", "8", "-p", "bilinear"), "bilinear"),
    (("in.png", "out.png", "--ensemble", "4", "-d"), "--downsample"),
    (("in.png", "out.png", "--ensemble", "2", "--devices", "0,1"), "more than one device"),
    (("validate", "--ensemble", "3", "folder"), "isn't a valid value for '--ensemble <N>'"),
    (("validate", "--ensemble", "8", "--devices", "0,1", "folder"), "more than one device"),
])
def test_cli_refuses_bad_ensemble_arguments(args, why):
    res = _cli(*args)
    assert res.returncode != 0
    assert why in res.stderr and "USAGE" in res.stderr, res.stderr
    assert not os.path.exists("out.png")


def test_cli_help_names_the_option():
    assert "--ensemble <N>" in _cli("--help").stdout
    assert "--ensemble <N>" in _cli("validate", "--help").stdout
