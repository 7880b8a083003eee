"""LR / HR pairs (include/srhip.h "Pairs") and the `--lr_folder`, `--val_lr_folder`, `-f` options of `rusty_sr train` / `validate`:
everything that needs no GPU -- help texts, argv rules (exit 2 before any device is touched), the pairing of files, and the new entry
points without a context.  The GPU side: test_gpu_pairs.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, gpu_available


def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=120)


def _folder(tmp_path, name, names=("0", "1"), ext=".png", size=(30, 42)):
    from PIL import Image
    d = tmp_path / name
    d.mkdir(parents=True, exist_ok=True)
    for i, n in enumerate(names):
        (d / n).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.random.default_rng(i).integers(0, 256, size + (3,), dtype=np.uint8)).save(d / f"{n}{ext}")
    return str(d)


def test_help_texts_name_the_new_options():
    r = _run("train", "--help")
    assert r.returncode == 0
    for opt in ("--lr_folder <DIR>", "--val_lr_folder <DIR>", "-f, --factor <2|3|4>", "[default: 3]"):
        assert opt in r.stdout, opt
    r = _run("validate", "--help")
    assert r.returncode == 0 and "--lr_folder <DIR>" in r.stdout


def test_train_pair_argv_rules(tmp_path):
    hr = _folder(tmp_path, "hr", size=(30, 42))
    lr = _folder(tmp_path, "lr", size=(10, 14))
    out = str(tmp_path / "o.rsr")
    r = _run("train", "--val_lr_folder", lr, out, hr)   # needs -v
    assert r.returncode == 2 and "--val_folder <VAL_FOLDER>" in r.stderr and "rusty_sr train" in r.stderr
    for v in ("5", "1", "x", "3.0", ""):
        r = _run("train", "-f", v, out, hr)
        assert r.returncode == 2 and "isn't a valid value for '--factor <2|3|4>'" in r.stderr, v
    r = _run("train", "--factor", "0", out, hr)
    assert r.returncode == 2
    for opt, name in (("-f", "--factor <2|3|4>"), ("--factor", "--factor <2|3|4>"), ("--lr_folder", "--lr_folder <DIR>"),
                      ("--val_lr_folder", "--val_lr_folder <DIR>")):
        r = _run("train", out, hr, opt)   # a missing value
        assert r.returncode == 2 and f"The argument '{name}' requires a value but none was supplied" in r.stderr, opt
    start = os.path.join(ROOT, "rusty_sr_amd", "res", "imagenet.rsr")
    for f in ("2", "4"):   # -f against a start file of another factor
        r = _run("train", "-s", start, "-f", f, out, hr)
        assert r.returncode == 2 and "--factor" in r.stderr and "factor 3" in r.stderr and "rusty_sr train" in r.stderr
    r = _run("train", "--lr_folder", str(tmp_path / "missing"), out, hr)
    assert r.returncode == 2 and "is not a folder" in r.stderr
    r = _run("train", "-v", hr, "--val_lr_folder", str(tmp_path / "missing"), out, hr)
    assert r.returncode == 2 and "is not a folder" in r.stderr
    assert not os.path.exists(out)


def test_validate_pair_argv_rules(tmp_path):
    hr = _folder(tmp_path, "hr")
    r = _run("validate", hr, "--lr_folder")
    assert r.returncode == 2 and "The argument '--lr_folder <DIR>' requires a value but none was supplied" in r.stderr
    r = _run("validate", "--lr_folder", str(tmp_path / "missing"), hr)
    assert r.returncode == 2 and "is not a folder" in r.stderr and "rusty_sr validate" in r.stderr


def test_a_missing_partner_is_named_before_any_device_is_touched(tmp_path):
    hr = _folder(tmp_path, "hr", names=("a", "b", "sub/c"))
    lr = _folder(tmp_path, "lr", names=("a", "x"), ext=".bmp", size=(10, 14))   # the extension is ignored; x has no partner: ignored
    out = str(tmp_path / "o.rsr")
    for args in (("train", "--lr_folder", lr, out, hr), ("validate", "--lr_folder", lr, hr),
                 ("train", "-v", hr, "--val_lr_folder", lr, out, hr)):
        r = _run(*args)
        assert r.returncode == 1 and "b.png has no LR partner in" in r.stderr and "a.png" not in r.stderr, r.stderr
        assert "HIP" not in r.stderr
    # -r applies to both folders: the partner of sub/c.png is sub/c.*
    _folder(tmp_path, "lr", names=("b",), ext=".bmp", size=(10, 14))
    r = _run("validate", "-r", "--lr_folder", lr, hr)
    assert r.returncode == 1 and "c.png has no LR partner in" in r.stderr
    assert not os.path.exists(out)


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU failure mode")
def test_pairs_without_a_gpu_refuse(tmp_path):
    hr = _folder(tmp_path, "hr", size=(30, 42))
    lr = _folder(tmp_path, "lr", size=(10, 14))
    out = tmp_path / "o.rsr"
    r = _run("train", "--lr_folder", lr, "--steps", "1", "--seed", "1", str(out), hr)
    assert r.returncode == 1 and "no HIP (gfx950) device available" in r.stderr and not out.exists()
    r = _run("train", "-f", "2", "--steps", "1", "--seed", "1", str(out), hr)
    assert r.returncode == 1 and "no HIP (gfx950) device available" in r.stderr and not out.exists()
    r = _run("validate", "--lr_folder", lr, hr)
    assert r.returncode == 1 and "no HIP (gfx950) device available" in r.stderr


def test_pair_entry_points_without_a_context():
    """Without a context the validation forms answer SR_E_INVALID, the backprop and session forms SR_E_NO_DEVICE where no device is
    present (SR_E_INVALID otherwise) -- as their pooled counterparts do; no output is written."""
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_INVALID if gpu_available() else _lib.SR_E_NO_DEVICE
    p = np.zeros(_lib.SR_NUM_PARAMS, np.float32)
    g = np.full(_lib.SR_NUM_PARAMS, 7.0, np.float32)
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lr8, hr8 = np.zeros((2, 2, 3), np.uint8), np.zeros((6, 6, 3), np.uint8)
    lrf, hrf = np.zeros((2, 2, 3), np.float32), np.zeros((6, 6, 3), np.float32)
    err, ne = C.c_double(5.0), C.c_size_t(3)
    assert L.sr_pair_validation_error_rgba8(None, lr8.ctypes.data_as(u8p), 3, hr8.ctypes.data_as(u8p), 3, 2, 2, 0, C.byref(err),
                                            C.byref(ne)) == _lib.SR_E_INVALID
    assert L.sr_pair_validation_error_f32(None, lrf.ctypes.data_as(fp), hrf.ctypes.data_as(fp), 2, 2, 0, C.byref(err),
                                          C.byref(ne)) == _lib.SR_E_INVALID
    assert L.sr_pair_validation_error_rgba8_dev(None, None, 3, None, 3, 2, 2, 0, None, None) == _lib.SR_E_INVALID
    assert L.sr_pair_backprop_rgba8(None, p.ctypes.data_as(fp), p.size, lr8.ctypes.data_as(u8p), 3, hr8.ctypes.data_as(u8p), 3, 1, 2, 2, 0,
                                    1.0, 0.0, C.byref(err), C.byref(ne), g.ctypes.data_as(fp)) == want
    assert L.sr_pair_backprop_f32(None, p.ctypes.data_as(fp), p.size, lrf.ctypes.data_as(fp), hrf.ctypes.data_as(fp), 1, 2, 2, 0, 1.0, 0.0,
                                  C.byref(err), C.byref(ne), g.ctypes.data_as(fp)) == want
    assert L.sr_pair_backprop_rgba8_dev(None, None, None, 3, None, 3, 1, 2, 2, 0, 1.0, 0.0, None, None, None) == want
    i = C.c_int(9)
    assert L.sr_train_add_pair(None, lr8.ctypes.data_as(u8p), 3, hr8.ctypes.data_as(u8p), 3, 2, 2, C.byref(i)) == want
    items = (_lib.TrainPairCrop * 1)()
    assert L.sr_train_step_pairs(None, items, 1, 64, 64) == want
    assert err.value == 5.0 and ne.value == 3 and i.value == 9 and (g == 7.0).all()


def test_pair_crop_structure_matches_the_header():
    """sr_train_pair_crop as ctypes lays it out is what a C compiler makes of the header's struct."""
    import re
    from rusty_sr_amd import _lib
    src = open(os.path.join(ROOT, "include", "srhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} sr_train_pair_crop;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    assert names == [f[0] for f in _lib.TrainPairCrop._fields_], names
    assert C.sizeof(_lib.TrainPairCrop) == 48 and _lib.TrainPairCrop.lr_px.offset == 8 and _lib.TrainPairCrop.y0.offset == 40
