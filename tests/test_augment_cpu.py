"""Training with random flips and rotations (include/srhip.h sr_train_step_aug / sr_train_step_pairs_aug, `rusty_sr train --augment`)
without a GPU: the header, the library's exports, the bindings, and the CLI's argument rules."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT, gpu_available

ENTRY_POINTS = {
    "sr_train_step_aug": r"\(sr_train\* t, const sr_train_crop\* items, const uint8_t\* members, int n, int crop_h, int crop_w\);",
    "sr_train_step_pairs_aug": r"\(sr_train\* t, const sr_train_pair_crop\* items, const uint8_t\* members, int n, int crop_lh, int crop_lw\);",
}


def _cli(*args, cwd=None):
    from rusty_sr_amd.build import build_host
    exe = build_host()
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # argument errors come before any device is touched
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=60, cwd=cwd)


def test_train_help_names_the_option():
    res = _cli("train", "--help")
    assert res.returncode == 0 and "--augment" in res.stdout


@pytest.mark.parametrize("args", [
    ("--augment", "in.png", "out.png"),
    ("in.png", "out.png", "--augment"),
    ("validate", "--augment", "folder"),
])
def test_cli_refuses_augment_outside_train(args, tmp_path):
    res = _cli(*args, cwd=tmp_path)  # (relative paths: nothing may be written there)
    assert res.returncode != 0
    assert "--augment" in res.stderr and "USAGE" in res.stderr, res.stderr
    assert os.listdir(tmp_path) == []


def test_header_declares_and_bindings_name_the_entry_points():
    text = open(os.path.join(ROOT, "include", "srhip.h")).read()
    rust = open(os.path.join(ROOT, "rust_host", "src", "srhip.rs")).read()
    from rusty_sr_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for name, args in ENTRY_POINTS.items():
        assert re.search(r"^int " + name + args, text, re.M), name
        assert hasattr(L, name), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == 6
        assert f"pub fn {name}(" in rust
    # the plain calls keep their declarations and item layouts
    assert "int sr_train_step(sr_train* t, const sr_train_crop* items, int n, int crop_h, int crop_w);" in text
    assert "int sr_train_step_pairs(sr_train* t, const sr_train_pair_crop* items, int n, int crop_lh, int crop_lw);" in text
    assert C.sizeof(_lib.TrainCrop) == 40 and C.sizeof(_lib.TrainPairCrop) == 48


def test_null_session_is_refused_like_the_other_session_calls():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_INVALID if gpu_available() else _lib.SR_E_NO_DEVICE
    items, pairs = (_lib.TrainCrop * 1)(), (_lib.TrainPairCrop * 1)()
    members = (C.c_uint8 * 1)(3)
    assert L.sr_train_step(None, items, 1, 192, 192) == want
    for m in (None, members):
        assert L.sr_train_step_aug(None, items, m, 1, 192, 192) == want
        assert L.sr_train_step_pairs_aug(None, pairs, m, 1, 64, 64) == want


def test_python_refuses_a_member_outside_0_to_7_before_the_library():
    import rusty_sr_amd as r
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            r.Trainer._members([(0, 0, 0), (0, 0, 0, bad)])
    assert r.Trainer._members([(0, 0, 0), (1, 2, 3)]) is None
    assert list(r.Trainer._members([(0, 0, 0), (0, 0, 0, 7)])) == [0, 7]
