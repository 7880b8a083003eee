"""The validation pass (include/srhip.h sr_validation_error_*, `rusty_sr validate`): everything about it that needs no GPU -- the
ABI in all four places, the CLI's argv rules, refusals before the device is touched.  The GPU side: test_gpu_validation.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

NEW = ["sr_read_validation_nodes", "sr_validation_error_f32", "sr_validation_error_rgba8", "sr_validation_error_rgba8_dev"]


def _read(*p):
    with open(os.path.join(*p)) as f:
        return f.read()


def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=120)


def test_validation_symbols_are_declared_exported_and_bound():
    from rusty_sr_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", _read(ROOT, "include", "srhip.h"), flags=re.S)
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes == _lib.SYMBOLS[name][1]
    assert "sr_validation" not in _read(ROOT, "include", "srhip_experimental.h")
    assert [len(_lib.SYMBOLS[n][1]) for n in NEW] == [5, 7, 8, 8]


def test_validation_rust_and_integration_declarations_match():
    def decls(text):
        return {m.group(1): re.sub(r"\s+", " ", m.group(0)) for m in re.finditer(r"pub fn (sr_validation\w+|sr_read_validation_nodes)\([^)]*\)[^;]*;", text)}
    rs, md = decls(_read(ROOT, "rust_host", "src", "srhip.rs")), decls(_read(ROOT, "INTEGRATION.md"))
    assert sorted(rs) == sorted(md) == NEW
    assert rs == md
    assert "d_err_sum: *mut f64" in rs["sr_validation_error_rgba8_dev"] and "n_elems: *mut usize" in rs["sr_validation_error_f32"]


def test_validation_refuses_null_arguments_before_the_gpu():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    err, n = C.c_double(), C.c_size_t()
    buf = (C.c_uint8 * 64)()
    assert L.sr_validation_error_rgba8(None, buf, 4, 4, 4, 0, C.byref(err), C.byref(n)) == _lib.SR_E_INVALID
    assert L.sr_validation_error_f32(None, None, 4, 4, 0, C.byref(err), C.byref(n)) == _lib.SR_E_INVALID
    assert L.sr_validation_error_rgba8_dev(None, None, 4, 4, 4, 0, None, None) == _lib.SR_E_INVALID
    assert L.sr_read_validation_nodes(None, None, 0, None, 0) == _lib.SR_E_INVALID


def test_validate_argv_rules(tmp_path):
    (tmp_path / "notes.txt").write_text("not an image")
    folder = str(tmp_path)
    r = _run("validate")
    assert r.returncode == 2 and "<VALIDATION_FOLDER>" in r.stderr
    r = _run("validate", str(tmp_path / "missing"))
    assert r.returncode == 2 and "not a folder" in r.stderr
    r = _run("validate", folder)  # a folder without a single image file (the .txt is skipped)
    assert r.returncode == 2 and "no image files" in r.stderr
    for bad in ("0", "-3", "x", "2.5", ""):
        r = _run("validate", "-m", bad, folder)
        assert r.returncode == 2 and "-val_max N must be a positive integer" in r.stderr, bad  # main.rs:225
    r = _run("validate", "-p", "bilinear", folder)
    assert r.returncode == 2 and "isn't a valid value" in r.stderr
    r = _run("validate", "-d", folder)
    assert r.returncode == 2 and "--downsample" in r.stderr
    r = _run("validate", "-p", "anime", "-c", "x.rsr", folder)
    assert r.returncode == 2 and "cannot be used with" in r.stderr
    r = _run("validate", "--bogus", folder)
    assert r.returncode == 2
    r = _run("validate", folder, folder)
    assert r.returncode == 2
    r = _run("validate", "--help")
    assert r.returncode == 0 and "--linearLoss" in r.stdout and "--val_max" in r.stdout and "--recurse" in r.stdout
    r = _run("--help")
    assert r.returncode == 0 and "rusty_sr validate" in r.stdout
    r = _run("train", "p.rsr", "folder")  # still declined
    assert r.returncode == 2 and "train" in r.stderr


def test_both_hosts_print_the_reference_line():
    cpp, rs = _read(ROOT, "rusty_sr_amd", "host", "main.cpp"), _read(ROOT, "rust_host", "src", "main.rs")
    for src in (cpp, rs):
        assert "Validation PSNR:\\t" in src  # main.rs:246
        assert '"validate"' in src and "--linearLoss" in src and "--val_max" in src and "--recurse" in src


def test_python_surface():
    import rusty_sr_amd as r
    assert callable(r.validation_psnr)
    for m in ("validation_error", "validation_error_dev", "validation_nodes"):
        assert callable(getattr(r.Engine, m))
    with pytest.raises(NotImplementedError):  # gradients stay out of scope
        r.sr_net(3, training=(0.0, False))
