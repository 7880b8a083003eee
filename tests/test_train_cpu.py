"""`rusty_sr train` and the training session's ABI (include/srhip.h sr_init_params, sr_train_*): everything that needs no GPU -- the
seeded initialisation against a restatement of its documented generator, and the CLI's argv rules.  The GPU side: test_gpu_train.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import grad_ref
from conftest import ROOT, gpu_available


def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args, cwd=None):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=120, cwd=cwd)


def _splitmix(seed):
    s = seed
    while True:
        s = (s + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        yield z ^ (z >> 31)


def _fan_in(shape):  # (out, ks, ks, in)
    return shape[1] * shape[2] * shape[3]


def restated_init(f, seed, upto=3000):
    """The generator include/srhip.h documents, for the first `upto` values (conv0 and the small segments after it)."""
    g = _splitmix(seed)
    out = []
    for name, (off, n, shape) in grad_ref.segments(f).items():
        for i in range(n):
            if len(out) >= upto:
                return np.array(out, dtype=np.float32)
            if name.endswith("_activ"):
                out.append(1.0 if i % 2 == 0 else 0.0)
            elif len(shape) == 1:
                out.append(0.0)
            else:
                std = (1.0 if name == "conv0" else 0.1) * math.sqrt(2.0 / _fan_in(shape))
                u1, u2 = (next(g) >> 11) * 2.0 ** -53, (next(g) >> 11) * 2.0 ** -53
                out.append(std * math.sqrt(-2.0 * math.log(1.0 - u1)) * math.cos(2.0 * math.pi * u2))
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("f", [2, 3, 4])
def test_init_params_is_seeded_and_sized(f):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    n = _lib.lib().sr_num_params_factor(f)
    a, b, c = r.init_params(f, 7), r.init_params(f, 7), r.init_params(f, 8)
    assert a.size == b.size == n == grad_ref.num_params(f)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, c)
    assert np.isfinite(a).all()
    want = restated_init(f, 7)
    assert np.array_equal(a[:want.size].view(np.uint32), want.view(np.uint32))
    # the buffer must hold every value
    import ctypes as C
    short = np.zeros(n - 1, np.float32)
    assert _lib.lib().sr_init_params(f, 1, short.ctypes.data_as(C.POINTER(C.c_float)), short.size) == _lib.SR_E_INVALID
    assert _lib.lib().sr_init_params(5, 1, short.ctypes.data_as(C.POINTER(C.c_float)), short.size) == _lib.SR_E_FACTOR


@pytest.mark.parametrize("f", [2, 3, 4])
def test_init_params_segments(f):
    import rusty_sr_amd as r
    p = r.init_params(f, 123)
    for name, (off, n, shape) in grad_ref.segments(f).items():
        seg = p[off:off + n].astype(np.float64)
        if name.endswith("_activ"):
            assert np.array_equal(seg, np.tile([1.0, 0.0], n // 2)), name
        elif len(shape) == 1:
            assert not seg.any(), name
        else:
            std = (1.0 if name == "conv0" else 0.1) * math.sqrt(2.0 / _fan_in(shape))
            assert abs(seg.std() / std - 1.0) < 0.05, (name, seg.std(), std)
            assert abs(seg.mean()) < 5 * std / math.sqrt(n), name


def test_train_help_and_top_level_help():
    r = _run("train", "--help")
    assert r.returncode == 0
    for opt in ("-l", "-r", "-s", "-v", "-m", "--steps", "--seed", "--device", "<PARAMETER_FILE>", "<TRAINING_FOLDER>"):
        assert opt in r.stdout, opt
    r = _run("--help")
    assert r.returncode == 0 and "rusty_sr train" in r.stdout


def _folder(tmp_path, name="train", n=2):
    from PIL import Image
    d = tmp_path / name
    d.mkdir()
    for i in range(n):
        Image.fromarray(np.random.default_rng(i).integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(d / f"{i}.png")
    return str(d)


def test_train_argv_rules(tmp_path):
    folder = _folder(tmp_path)
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("no images here")
    out = str(tmp_path / "o.rsr")
    r = _run("train", "-m", "3", out, folder)  # clap: -m requires -v
    assert r.returncode == 2 and "--val_folder" in r.stderr and "rusty_sr train" in r.stderr
    r = _run("train", "-v", folder, "-m", "x", out, folder)
    assert r.returncode == 2 and "-val_max N must be a positive integer" in r.stderr  # main.rs:225
    r = _run("train", "-v", folder, "-m", "0", out, folder)
    assert r.returncode == 2
    r = _run("train", out, str(tmp_path / "missing"))
    assert r.returncode == 2 and "rusty_sr train" in r.stderr
    r = _run("train", out, str(empty))
    assert r.returncode == 2 and "no image files" in r.stderr
    r = _run("train", out, folder, "extra")
    assert r.returncode == 2 and "wasn't expected" in r.stderr
    r = _run("train", out)
    assert r.returncode == 2 and "required arguments" in r.stderr
    r = _run("train", "--steps", "0", out, folder)
    assert r.returncode == 2
    r = _run("train", "--bogus", out, folder)
    assert r.returncode == 2
    r = _run("train", "-s", str(tmp_path / "nope.rsr"), out, folder)
    assert r.returncode == 1 and "Error opening start parameter file" in r.stderr  # main.rs:192
    assert not os.path.exists(out)


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU failure mode")
def test_train_without_a_gpu_refuses(tmp_path):
    folder = _folder(tmp_path)
    out = tmp_path / "o.rsr"
    r = _run("train", "--steps", "1", "--seed", "1", str(out), folder)
    assert r.returncode == 1 and "no HIP (gfx950) device available" in r.stderr
    assert "Beginning Training" not in r.stdout and not out.exists()


def test_session_entry_points_without_a_context():
    """Every session entry point refuses a missing session; without a device the answer is SR_E_NO_DEVICE."""
    import ctypes as C
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_INVALID if gpu_available() else _lib.SR_E_NO_DEVICE
    p = np.zeros(_lib.SR_NUM_PARAMS, np.float32)
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    t = C.c_void_p()
    assert L.sr_train_create(C.byref(t), None, fp, p.size, 0, 1e-6, 2e-3, 0.95, 0.995, 1e-7, 0) == want
    assert L.sr_set_params(None, fp, p.size) == want
    n = C.c_size_t()
    assert L.sr_train_sync(None, None, 0, C.byref(n)) == want
    assert L.sr_train_params(None, fp, p.size) == want
    items = (_lib.TrainCrop * 1)()
    assert L.sr_train_step(None, items, 1, 192, 192) == want
    L.sr_train_destroy(None)
