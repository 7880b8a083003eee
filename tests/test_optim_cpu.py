"""The optimiser's additions without a GPU (include/srhip.h "Optimiser"): the restated norm against math.fsum, sr_lr_at against its
numpy restatement, the schedule parser, the state-file parser as a stand-alone program, the CLI's refusals and the null-context answers."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import optim_ref
from conftest import ROOT, gpu_available

CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


# ---- the restated sum
@pytest.mark.parametrize("n", optim_ref.NORM_SIZES + (117484, 130459, 148624))
def test_restated_sum_is_within_its_bound_of_fsum(n):
    """Every square is exact in f64 and positive, and each addition errs by at most 2^-53 of its result; a term passes through far
    fewer than n additions (8 butterfly levels, 3 wave sums, at most n / 65536 + 1 partial rounds, 11 more), so the restated S is well
    within n 2^-53 relative of the exactly rounded sum."""
    for name, g in optim_ref.norm_vectors(n).items():
        exact = math.fsum(float(x) * float(x) for x in g.astype(np.float64))
        got = float(optim_ref.sumsq(g))
        assert abs(got - exact) <= n * 2.0 ** -53 * exact, (n, name, got, exact)
        if name == "zero":
            assert got == 0.0


def test_wave_sum_is_the_butterfly():
    v = np.random.default_rng(3).standard_normal(64)
    w = v.copy()
    for off in (32, 16, 8, 4, 2, 1):
        w = np.array([w[i] + w[i ^ off] for i in range(64)])
    got = optim_ref.wave_sum(v)
    assert np.array_equal(got, w) and np.all(got == got[0])


def test_scale_rule():
    S = np.float64(25.0)
    assert optim_ref.norm_rule(S, 0.0) == (np.float32(1.0), 0)            # clipping off
    assert optim_ref.norm_rule(S, 5.0) == (np.float32(1.0), 0)            # norm == clip: not above it
    assert optim_ref.norm_rule(S, 10.0) == (np.float32(1.0), 0)
    assert optim_ref.norm_rule(S, 2.5) == (np.float32(0.5), 0)
    assert optim_ref.norm_rule(np.float64(0.0), 1.0) == (np.float32(1.0), 0)
    assert optim_ref.norm_rule(np.float64(np.inf), 1.0) == (np.float32(0.0), 1)
    scale, skip = optim_ref.norm_rule(np.float64(np.nan), 1.0)
    assert scale == np.float32(1.0) and skip == 1
    g = np.array([1.0, np.nan, 2.0], np.float32)
    assert optim_ref.grad_norm(g, 1.0)["skip"] == 1
    g[1] = -np.inf
    assert optim_ref.grad_norm(g, 1.0)["skip"] == 1


def test_ema_rule_rounds_each_operation():
    e, p = np.float32([1.0, 3.0]), np.float32([2.0, 1e-3])
    d = np.float32(0.99)
    want = np.float32([np.float32(d * e[k]) + np.float32((np.float32(1.0) - d) * p[k]) for k in range(2)])
    assert np.array_equal(optim_ref.ema(e, p, 0.99), want)


# ---- sr_lr_at
def _ulp_apart(a, b):
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


SCHEDULES = [("constant", dict()), ("constant", dict(warmup=7)), ("step:5:0.5", dict()), ("step:13:0.9", dict(warmup=4)),
             ("cosine:40", dict()), ("cosine:64:1e-4", dict(warmup=10)), ("cosine:1", dict())]


@pytest.mark.parametrize("text,kw", SCHEDULES)
def test_lr_at_matches_the_restatement(text, kw):
    """Equal for constant and warm-up alone; within one f32 ulp for step and cosine (libm's and numpy's pow / cos may differ in the last
    f64 bit, and the one rounding to f32 may then fall either way)."""
    import rusty_sr_amd as r
    base = 2e-3
    s = r.parse_lr_schedule(text, base, kw.get("warmup", 0))
    parts = text.split(":")
    ref = dict(kw)
    total = 20
    if parts[0] == "step":
        ref.update(every=int(parts[1]), gamma=float(parts[2]))
    if parts[0] == "cosine":
        total = int(parts[1])
        ref.update(total=total, min_lr=float(parts[2]) if len(parts) > 2 else 0.0)
    for t in range(1, 3 * total + 1):
        got, want = np.float32(r.lr_at(s, t)), optim_ref.lr_at(parts[0], base, t, **ref)
        if parts[0] == "constant":
            assert got == want, (text, t, got, want)
        else:
            assert _ulp_apart(got, want) <= 1, (text, t, got, want)
    if parts[0] == "cosine":   # the ends: the base rate at step 1 (after warm-up), MIN from step TOTAL + 1 on
        assert np.float32(r.lr_at(s, 3 * total)) == np.float32(ref["min_lr"])
        if not kw.get("warmup"):
            assert np.float32(r.lr_at(s, 1)) == np.float32(base)
    if kw.get("warmup"):
        assert np.float32(r.lr_at(s, 1)) < np.float32(r.lr_at(s, kw["warmup"]))


def test_lr_at_refusals_leave_the_output_untouched():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    out = C.c_float(123.0)
    good = _lib.LrSchedule(_lib.SR_LR_COSINE, 2e-3, 0, 0, 0.0, 10, 0.0)
    assert L.sr_lr_at(None, 1, C.byref(out)) == _lib.SR_E_INVALID
    assert L.sr_lr_at(C.byref(good), 1, None) == _lib.SR_E_INVALID
    assert L.sr_lr_at(C.byref(good), 0, C.byref(out)) == _lib.SR_E_INVALID
    bad = [dict(kind=7), dict(base=float("nan")), dict(base=float("inf")), dict(base=-1.0), dict(warmup=-1), dict(total=0), dict(min_lr=-1.0),
           dict(min_lr=1.0), dict(min_lr=float("nan")), dict(kind=_lib.SR_LR_STEP, every=0, gamma=0.5), dict(kind=_lib.SR_LR_STEP, every=2, gamma=0.0),
           dict(kind=_lib.SR_LR_STEP, every=2, gamma=1.5), dict(kind=_lib.SR_LR_STEP, every=2, gamma=float("nan"))]
    for change in bad:
        s = _lib.LrSchedule(_lib.SR_LR_COSINE, 2e-3, 0, 0, 0.0, 10, 0.0)
        for k, v in change.items():
            setattr(s, k, v)
        assert L.sr_lr_at(C.byref(s), 1, C.byref(out)) == _lib.SR_E_INVALID, change
    assert out.value == 123.0
    assert L.sr_lr_at(C.byref(good), 1, C.byref(out)) == _lib.SR_OK and np.float32(out.value) == np.float32(2e-3)


def test_parse_lr_schedule_refusals_name_the_option():
    import rusty_sr_amd as r
    for text in ("", "linear", "step", "step:5", "step:0:0.5", "step:5:0", "step:5:1.5", "step:x:0.5", "step:5:0.5:1", "cosine", "cosine:0",
                 "cosine:-3", "cosine:10:1", "cosine:10:-1e-4", "cosine:10:nan", "cosine:1.5", "constant:1"):
        with pytest.raises(ValueError) as e:
            r.parse_lr_schedule(text, 2e-3)
        assert "--lr-schedule" in str(e.value), text
    for base in (float("nan"), float("inf"), -1.0, "x"):
        with pytest.raises(ValueError) as e:
            r.parse_lr_schedule("constant", base)
        assert "--lr:" in str(e.value)
    for warm in (-1, 1.5, "3"):
        with pytest.raises(ValueError) as e:
            r.parse_lr_schedule("constant", 2e-3, warm)
        assert "--warmup" in str(e.value)
    s = r.parse_lr_schedule("cosine:200:1e-5", 1e-3, 10)
    assert (s.kind, s.total, s.warmup) == (2, 200, 10) and np.float32(s.min_lr) == np.float32(1e-5)


# ---- entry points without a context
def test_optimiser_entry_points_without_a_context():
    """Every new entry point refuses a missing context or session: SR_E_INVALID, or SR_E_NO_DEVICE where the machine has no device (as
    sr_adam_step_dev answers)."""
    from rusty_sr_amd import _lib
    L = _lib.lib()
    want = _lib.SR_E_INVALID if gpu_available() else _lib.SR_E_NO_DEVICE
    buf = np.zeros(64, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    vp = C.c_void_p(buf.ctypes.data)
    assert L.sr_grad_norm_dev(None, vp, 4, 1.0, vp, None) == want
    assert L.sr_adam_step_clipped_dev(None, vp, vp, vp, vp, 4, 1, 2e-3, 0.95, 0.995, 1e-7, vp, None, 0.0, None, None) == want
    assert L.sr_train_set_optim(None, 1.0, 0.99) == want
    assert L.sr_train_set_lr(None, 1e-3) == want
    assert L.sr_train_ema(None, fp, buf.size) == want
    step, skipped, n = C.c_longlong(), C.c_longlong(), C.c_size_t()
    assert L.sr_train_get_state(None, fp, fp, fp, buf.size, C.byref(step), C.byref(skipped)) == want
    assert L.sr_train_set_state(None, fp, fp, fp, buf.size, 0, 0) == want
    assert L.sr_train_sync_stats(None, None, 0, C.byref(n)) == want
    assert not buf.any()


# ---- the state file's parser, as a program of its own
@pytest.mark.parametrize("sanitize", [False, True])
def test_state_parser_program(tmp_path, sanitize):
    exe = str(tmp_path / ("train_state_san" if sanitize else "train_state"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "train_state.cpp"),
                           os.path.join(ROOT, "rusty_sr_amd", "host", "train_state.cpp"), "-o", exe])
    res = subprocess.run([exe, str(tmp_path / "s.state")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr, res.stderr   # (a sanitizer report ends the program with a status of its own)
    lines = res.stdout.strip().split("\n")
    header = 320   # srstate::kHeaderBytes
    for k, (name, arrays) in enumerate((("averaged", 3), ("plain", 2))):
        size = header + 37 * 4 * arrays
        assert lines[3 * k] == f"roundtrip {name} ok"
        assert lines[3 * k + 1] == f"truncations refused {size + 1} of {size + 1}"
        assert lines[3 * k + 2] == f"header flips refused {8 * header} of {8 * header}"
    rest = lines[6:]
    assert rest[:7] == [f"count {n} refused" for n in (0, 38, 1 << 30, 1 << 61, (1 << 62) + 37, 0x5555555555555555 + 37, 2 ** 64 - 1)]
    assert rest[7:11] == ["count 37 ok", "step -1 refused", "encode short moments refused", "encode long spec refused"]
    assert rest[11] == "differing: '' --seed --loss --lr --lr-schedule --warmup --clip --ema"
    assert rest[12:] == ["file ok, temporary gone", "missing file refused"]


# ---- the CLI's refusals: status 2 and the option's name, with no GPU in the machine
def _cli():
    from rusty_sr_amd.build import build_host
    return build_host()


def _run(*args):
    return subprocess.run([_cli(), *args], capture_output=True, text=True, timeout=120)


def _folder(tmp_path, name="train", n=2):
    from PIL import Image
    d = tmp_path / name
    d.mkdir()
    for i in range(n):
        Image.fromarray(np.random.default_rng(i).integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(d / f"{i}.png")
    return str(d)


def _fnv1a(data: bytes) -> int:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def state_bytes(n_params, step=100, seed=7, factor=3, n_files=2, loss_kind=0, loss_eps=1e-3, lr=2e-3, sched_kind=0, warmup=0, every=0,
                gamma=0.0, total=0, min_lr=0.0, clip=0.0, ema=0.0, flags=0, degrade=b"", params_hash=0):
    """The state file of rusty_sr_amd/host/train_state.hpp, version 1, written from its description: zero moments, generators at 1..6.
    params_hash: the FNV-1a of the parameter file's bytes it belongs to."""
    import struct
    head = b"RSRSTATE" + struct.pack("<IIiI", 1, 320, factor, flags)
    head += struct.pack("<QqqQQQQQQQQQ", n_params, step, 0, seed, 1, 2, 3, 0, 5, 0, n_files, params_hash)
    head += struct.pack("<iffi", loss_kind, loss_eps, lr, sched_kind) + struct.pack("<qqdq", warmup, every, gamma, total)
    head += struct.pack("<fffI", min_lr, clip, ema, 0)
    head += degrade.ljust(128, b"\0")
    assert len(head) == 312
    head += struct.pack("<Q", _fnv1a(head))
    return head + bytes(4 * n_params * (3 if ema > 0 else 2))


def test_cli_refuses_malformed_optimiser_options(tmp_path):
    folder = _folder(tmp_path)
    out = str(tmp_path / "o.rsr")
    bad = [("--lr", "x"), ("--lr", "-1"), ("--lr", "nan"), ("--lr", "1e99"), ("--lr-schedule", "linear"), ("--lr-schedule", "step:0:0.5"),
           ("--lr-schedule", "step:5:1.5"), ("--lr-schedule", "step:5"), ("--lr-schedule", "cosine:0"), ("--lr-schedule", "cosine:10:1"),
           ("--lr-schedule", "cosine:x"), ("--lr-schedule", ""), ("--warmup", "-1"), ("--warmup", "1.5"), ("--warmup", "x"), ("--clip", "-1"),
           ("--clip", "inf"), ("--clip", "x"), ("--clip", "1e-50"), ("--lr", "1e-50"), ("--ema", "1e-50"), ("--ema", "1"), ("--ema", "1.5"), ("--ema", "-0.1"), ("--ema", "x")]
    for opt, val in bad:
        r = _run("train", "--steps", "1", opt, val, out, folder)
        assert r.returncode == 2 and opt in r.stderr and "rusty_sr train" in r.stderr, (opt, val, r.stderr)
    for opt in ("--lr", "--lr-schedule", "--warmup", "--clip", "--ema"):
        r = _run("train", out, folder, opt)
        assert r.returncode == 2 and opt in r.stderr and "requires a value" in r.stderr
    assert not os.path.exists(out)


def test_cli_refuses_the_optimiser_options_elsewhere(tmp_path):
    folder = _folder(tmp_path)
    img = os.path.join(folder, "0.png")
    for opt, val in (("--lr", "1e-3"), ("--lr-schedule", "cosine:10"), ("--warmup", "3"), ("--clip", "1"), ("--ema", "0.9"), ("--resume", None)):
        extra = [opt] + ([val] if val else [])
        for args in (["validate", *extra, folder], ["video", *extra, "-", "-"], [*extra, img, str(tmp_path / "o.png")]):
            r = _run(*args)
            assert r.returncode == 2 and f"'{opt}'" in r.stderr and "'train' subcommand" in r.stderr, (args, r.stderr)
    assert not os.path.exists(tmp_path / "o.png")


def test_cli_resume_refusals_name_the_file_or_the_option(tmp_path):
    import rusty_sr_amd as r
    folder = _folder(tmp_path)
    out = tmp_path / "o.rsr"
    base = ["train", "--resume", "--steps", "200", "--seed", "7"]
    res = _run(*base, str(out), folder)
    assert res.returncode == 2 and str(out) in res.stderr and "parameter file" in res.stderr
    p = r.init_params(3, 7)
    out.write_bytes(r.rsr.encode(p))
    res = _run(*base, str(out), folder)
    assert res.returncode == 2 and str(out) + ".state" in res.stderr and "state file" in res.stderr
    state = tmp_path / "o.rsr.state"
    good = lambda n: state_bytes(n, params_hash=_fnv1a(out.read_bytes()))   # noqa: E731  (the state that belongs to `out`)
    state.write_bytes(good(p.size))
    # the same options pass every check that needs no device (what follows is the device's to refuse, or the run itself)
    res = _run(*base, str(out), folder)
    assert res.returncode != 2 or "--resume" not in res.stderr, res.stderr
    if not gpu_available():
        assert res.returncode == 1 and "no HIP (gfx950) device available" in res.stderr
    out.write_bytes(r.rsr.encode(p))   # (a run on a GPU has replaced both)
    state.write_bytes(good(p.size))
    for extra, named in ((["--seed", "8"], "--seed"), (["--loss", "l1"], "--loss"), (["--loss", "charbonnier:0.01"], "--loss"), (["--lr", "1e-3"], "--lr"),
                         (["--lr-schedule", "cosine:200"], "--lr-schedule"), (["--warmup", "10"], "--warmup"), (["--clip", "1"], "--clip"),
                         (["--ema", "0.99"], "--ema"), (["--augment"], "--augment"), (["-l"], "--linearLoss"), (["--degrade", "blur=1"], "--degrade")):
        args = [a for a in base if extra[0] != "--seed" or a not in ("--seed", "7")]
        res = _run(*args, *extra, str(out), folder)
        assert res.returncode == 2 and f"'{named}' differs" in res.stderr, (extra, res.stderr)
    res = _run("train", "--resume", "--steps", "100", "--seed", "7", str(out), folder)   # --steps is the total
    assert res.returncode == 2 and "--steps" in res.stderr
    res = _run(*base, "-s", str(out), str(out), folder)
    assert res.returncode == 2 and "--resume" in res.stderr and "--start" in res.stderr
    for blob in (state.read_bytes()[:-1], state.read_bytes()[:100], b"", good(p.size - 1)):
        state.write_bytes(blob)
        res = _run(*base, str(out), folder)
        assert res.returncode == 2 and str(state) in res.stderr, res.stderr
    flipped = bytearray(good(p.size))
    flipped[40] ^= 1
    state.write_bytes(bytes(flipped))
    res = _run(*base, str(out), folder)
    assert res.returncode == 2 and "checksum" in res.stderr
    assert r.rsr.decode(out.read_bytes()).size == p.size   # nothing was overwritten


def test_cli_resume_refuses_a_parameter_file_of_another_checkpoint(tmp_path):
    """The state file names its parameter file by the FNV-1a of that file's bytes.  A .rsr of the same length beside it -- what a run ended
    between the two writes leaves, or a file put there since -- is refused with status 2 and both names, before a device is touched, and
    nothing is overwritten; the file the state was written with passes that check."""
    import rusty_sr_amd as r
    folder = _folder(tmp_path)
    out, state = tmp_path / "o.rsr", tmp_path / "o.rsr.state"
    base = ["train", "--resume", "--steps", "200", "--seed", "7", str(out), folder]
    mine, other = r.rsr.encode(r.init_params(3, 7)), r.rsr.encode(r.init_params(3, 8))
    assert len(mine) == len(other) and mine != other
    blob = state_bytes(r.init_params(3, 7).size, params_hash=_fnv1a(mine))
    for beside in (other, mine[:-1] + bytes([mine[-1] ^ 1])):
        out.write_bytes(beside)
        state.write_bytes(blob)
        res = _run(*base)
        assert res.returncode == 2 and "--resume" in res.stderr and str(out) in res.stderr and str(state) in res.stderr and "checksum" in res.stderr, res.stderr
        assert out.read_bytes() == beside and state.read_bytes() == blob
    out.write_bytes(mine)
    res = _run(*base)
    assert res.returncode != 2 or "--resume" not in res.stderr, res.stderr
