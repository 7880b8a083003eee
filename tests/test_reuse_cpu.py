"""The row reuse of the frame stream without a GPU: the planner (sr_video_reuse_plan, rusty_sr_amd/csrc/sr_plan.cpp) against its numpy
restatement (tests/reuse_ref.py) and against properties taken straight from the rule of include/srhip.h, a stand-alone C++ program that
drives it over the same families (also under ASan + UBSan), the ABI in its four places, and the refusals of `--reuse` that the CLI decides
before it touches a device.  The kernel and the session are held to this in tests/test_gpu_reuse.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reuse_ref
from conftest import ROOT

HALO = 7
HEIGHTS = (1, 2, 7, 8, 15, 16, 31, 64, 65, 128, 1080)
SUBS = {"420": reuse_ref.SUB_420, "444": reuse_ref.SUB_444, "422": reuse_ref.SUB_422}
NEW = ("sr_rows_differ_dev", "sr_video_reuse_plan", "sr_video_set_reuse", "sr_video_get_reuse_stats")
CLI = os.path.join(ROOT, "rusty_sr_amd", "bin", "rusty_sr")


def cases():
    """(sub, h, dirty plane rows) of every family: empty, full, a single dirty luma row at every position for h <= 65 (a spread of
    positions above), a single dirty chroma row of either plane at every position at every height, seeded random masks of 1-3 dirty plane rows."""
    rng = np.random.default_rng(20260)
    out = []
    for sub in SUBS.values():
        for h in HEIGHTS:
            ch = reuse_ref.chroma_rows(sub, h)
            rows = h + 2 * ch
            out.append((sub, h, ()))
            out.append((sub, h, tuple(range(rows))))
            every = range(h) if h <= 65 else sorted({0, 1, 6, 7, 8, 13, 14, 15, h // 2, h // 2 + 1, h - 16, h - 15, h - 14, h - 9, h - 8, h - 7, h - 2, h - 1})
            out += [(sub, h, (y, )) for y in every]
            out += [(sub, h, (h + p * ch + c, )) for p in (0, 1) for c in range(ch)]
            for _ in range(40 if h >= 64 else 12):
                k = int(rng.integers(1, 4))
                out.append((sub, h, tuple(sorted(int(r) for r in rng.choice(rows, size=min(k, rows), replace=False)))))
    return out


CASES = cases()


def flags_of(sub, h, dirty):
    f = np.zeros(h + 2 * reuse_ref.chroma_rows(sub, h), np.uint32)
    f[list(dirty)] = 1
    return f


def tap_dirty(flags, sub, h):
    """The RGB-dirty luma rows straight from the tap rule of include/srhip.h, not through reuse_ref: row 2i reads C[i - 1] and C[i], row
    2i + 1 reads C[i] and C[i + 1], indices clamped to the plane; 4:2:2 and 4:4:4 read their own row."""
    ch = (h + 1) // 2 if sub == reuse_ref.SUB_420 else h
    out = []
    for y in range(h):
        if sub == reuse_ref.SUB_420:
            i = y // 2
            taps = (max(0, i - 1), i) if y % 2 == 0 else (i, min(ch - 1, i + 1))
        else:
            taps = (y, y)
        if flags[y] or any(flags[h + p * ch + c] for p in (0, 1) for c in taps):
            out.append(y)
    return out


def test_the_families_are_there():
    assert len(CASES) > 8000
    assert {h for _, h, _ in CASES} == set(HEIGHTS) and {s for s, _, _ in CASES} == set(SUBS.values())


def test_plan_equals_the_restatement_and_holds_its_properties():
    from rusty_sr_amd import video_reuse_plan
    partial = 0
    for sub, h, dirty in CASES:
        flags = flags_of(sub, h, dirty)
        want = reuse_ref.plan(flags, sub, h)
        got = video_reuse_plan(flags, sub, h)
        assert got == want, (sub, h, dirty, got, want)
        # ---- the properties, from the rule alone
        assert len(got) <= 4
        assert all(0 <= a < b <= h for a, b in got) and all(got[i][1] < got[i + 1][0] for i in range(len(got) - 1)), got
        for a, b in got:
            assert a % 2 == 0 and (b % 2 == 0 or b == h), (h, got)
            assert not 0 < a < HALO and not h - HALO < b < h, (h, got)
        covered = np.zeros(h, bool)
        for a, b in got:
            covered[a:b] = True
        for y in tap_dirty(flags, sub, h):
            assert covered[max(0, y - HALO):y + HALO + 1].all(), (sub, h, dirty, got)
        if not dirty:
            assert got == []
        if len(dirty) == len(flags):
            assert got == [(0, h)]
        # ---- not vacuous: three dirty plane rows never cost a tall frame whole (at most 3 x 21 rows + 3 x 14 margin rows = 105 < 128)
        if h >= 128 and 1 <= len(dirty) <= 3:
            assert got and got != [(0, h)] and sum(b - a for a, b in got) < h, (sub, h, dirty, got)
            partial += 1
    assert partial > 200


def test_plan_merges_and_caps_as_stated():
    from rusty_sr_amd import video_reuse_plan

    def plan(h, *rows):
        return video_reuse_plan(flags_of(reuse_ref.SUB_444, h, rows), "444", h)

    assert plan(1080, 500) == [(492, 508)]                      # one row: SR_HALO either side, edges even
    assert plan(1080, 501) == [(494, 510)]
    assert plan(1080, 3) == [(0, 12)] and plan(1080, 12) == [(0, 20)] and plan(1080, 1066) == [(1058, 1080)]  # no edge inside SR_HALO of an image edge
    assert plan(1080, 100, 129) == [(92, 108), (122, 138)]      # 14 clean rows between the bands: apart
    assert plan(1080, 100, 127) == [(92, 136)]                  # 12: merged
    five = (100, 300, 340, 600, 900)                            # five bands: the smallest gap goes
    assert plan(1080, *five) == [(92, 108), (292, 348), (592, 608), (892, 908)]
    assert plan(1080, 100, 200, 300, 400, 500) == [(92, 208), (292, 308), (392, 408), (492, 508)]  # equal gaps: the pair nearer the top
    assert plan(64, 30) == [(22, 38)] and plan(64, 10, 50) == [(0, 64)]  # 16 + 14 < 64; [0, 18) and [42, 64) with 2 x 14 reach it
    assert video_reuse_plan(flags_of(reuse_ref.SUB_420, 64, (64 + 10, )), "420", 64) == [(12, 30)]  # chroma row 10: luma rows 19 .. 22


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_planner_program(tmp_path, sanitize):
    """tests/c/reuse_plan_check.cpp: g++ alone, sr_plan.cpp alone -- the planner needs no HIP -- over every case; it checks each plan's
    invariants itself and prints it, and the plans equal the restatement's."""
    exe = str(tmp_path / "reuse_plan_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "reuse_plan_check.cpp"),
                           os.path.join(ROOT, "rusty_sr_amd", "csrc", "sr_plan.cpp"), "-o", exe])
    text = "".join(f"{sub} {h} {' '.join(map(str, dirty))}\n" for sub, h, dirty in CASES)
    res = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(CASES) and f"{len(CASES)} cases" in res.stderr
    for (sub, h, dirty), line in zip(CASES, lines):
        want = reuse_ref.plan(flags_of(sub, h, dirty), sub, h)
        assert [int(x) for x in line.split()] == [len(want)] + [e for band in want for e in band], (sub, h, dirty, line)


def test_restatement_helpers():
    """frame_flags and frame_stats, which the GPU test predicts a session with."""
    a = np.arange(6 * 4 + 2 * 3 * 2, dtype=np.uint8)
    b = a.copy()
    b[5] ^= 1       # Y row 1
    b[24 + 2] ^= 1  # Cb row 1
    assert reuse_ref.frame_flags(a, b, reuse_ref.SUB_420, 6, 4).tolist() == [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert reuse_ref.frame_stats([], 64) == {"frames": 1, "frames_reused": 1, "frames_partial": 0, "frames_full": 0, "rows_total": 64, "rows_computed": 0, "bands": 0}
    assert reuse_ref.frame_stats([(0, 64)], 64)["frames_full"] == 1 and reuse_ref.frame_stats([(0, 64)], 64)["bands"] == 0
    assert reuse_ref.frame_stats([(0, 12), (40, 64)], 64) == {"frames": 1, "frames_reused": 0, "frames_partial": 1, "frames_full": 0, "rows_total": 64,
                                                              "rows_computed": 36, "bands": 2}


def test_entry_points_are_declared_and_exported():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    header_text = open(os.path.join(ROOT, "include", "srhip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    rust = open(os.path.join(ROOT, "rust_host", "src", "srhip.rs")).read()
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        assert f"pub fn {name}(" in rust and f"pub fn {name}(" in md, name
    assert re.search(r"SR_VIDEO_REUSE_OFF = 0, SR_VIDEO_REUSE_ROWS = 1", header) and (_lib.SR_VIDEO_REUSE_OFF, _lib.SR_VIDEO_REUSE_ROWS) == (0, 1)
    assert int(re.search(r"#define SR_REUSE_MAX_BANDS (\d+)", header).group(1)) == _lib.SR_REUSE_MAX_BANDS == reuse_ref.MAX_BANDS == 4
    assert C.sizeof(_lib.RowBand) == 8 and C.sizeof(_lib.VideoReuseStats) == 56
    assert "pub struct SrRowBand" in rust and "pub struct SrVideoReuseStats" in rust
    assert "there is no temporal processing" not in header_text


def test_entry_points_without_a_context_or_a_session():
    from rusty_sr_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint32 * 16)()
    p = C.cast(buf, C.c_void_p)
    INV = _lib.SR_E_INVALID
    assert L.sr_rows_differ_dev(None, p, p, 1, 4, p, None) == INV
    assert L.sr_video_set_reuse(None, 1) == INV
    st = _lib.VideoReuseStats()
    assert L.sr_video_get_reuse_stats(None, C.byref(st)) == INV
    bands, n = (_lib.RowBand * 4)(), C.c_int(9)
    assert L.sr_video_reuse_plan(None, 1, 4, bands, 4, C.byref(n)) == INV and n.value == 0
    assert L.sr_video_reuse_plan(buf, 1, 0, bands, 4, C.byref(n)) == INV
    assert L.sr_video_reuse_plan(buf, 3, 4, bands, 4, C.byref(n)) == INV
    assert L.sr_video_reuse_plan(buf, 1, 4, bands, 0, C.byref(n)) == INV
    assert L.sr_video_reuse_plan(buf, 1, 4, bands, 4, None) == INV


def _cli(stdin_bytes, *args):
    from rusty_sr_amd.build import build_host
    build_host()
    return subprocess.run([CLI, *args], input=stdin_bytes, capture_output=True, timeout=120)


def test_cli_refuses_reuse_outside_video_before_touching_a_gpu():
    for args in (("--reuse", "a.png", "b.png"), ("a.png", "b.png", "--reuse"), ("train", "--reuse", "p.rsr", "folder"), ("validate", "--reuse", "folder")):
        res = _cli(b"", *args)
        assert res.returncode == 2 and b"'--reuse'" in res.stderr and b"'video'" in res.stderr and res.stdout == b"", (args, res.stderr)
    res = _cli(b"", "video", "--help")
    assert res.returncode == 0 and b"--reuse" in res.stderr
    res = _cli(b"not a stream\n", "video", "--reuse", "-", "-")  # the option itself is taken: the stream is what is refused
    assert res.returncode == 2 and b"YUV4MPEG2" in res.stderr and b"--reuse" not in res.stderr
