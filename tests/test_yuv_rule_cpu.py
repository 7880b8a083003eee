"""The one rule of the video path's two formats (rusty_sr_amd/csrc/sr_yuv_rule.h -- the header the conversion kernels and their host side
compile) through a plain C++ program, tests/c/yuv_rule_dump.cpp: every constant it forms equals tests/yuv_ref.py's and tests/yuv16_ref.py's
bit for bit, its frame sizes are theirs, and each of the two validators refuses what its format does not hold.  No GPU: this is the part
of "8-bit frames are deep frames at depth 8" that can be proved without one; the kernels are held to the same two restatements in
tests/test_gpu_video.py and tests/test_gpu_video_deep.py."""
import os
import struct
import subprocess

import pytest

import yuv16_ref
import yuv_ref
from conftest import ROOT

SUBS = {0: "420", 1: "444", 2: "422"}            # include/srhip.h SR_YUV_420, SR_YUV_444, SR_YUV_422
SITINGS = {0: "center", 1: "left"}
MATRICES = {0: "bt601", 1: "bt709", 2: "bt2020"}
RANGES = {0: "limited", 1: "full"}
SHAPES = ((1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (17, 13), (1080, 1920), (3241, 5761))   # yuv_rule_dump.cpp SHAPES
FIELDS = ("kr", "kb", "kg", "cr2", "cb2", "ir", "ib", "ig", "oy", "mid", "sy", "sc", "ky", "kc", "ylo", "yhi", "clo", "chi")


def bits(v):
    return struct.pack("<d", float(v))


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("yuv_rule_dump_san" if sanitize else "yuv_rule_dump"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "c", "yuv_rule_dump.cpp"), "-o", exe])
    return exe


def expected(width, sub, siting, matrix, range_, depth):
    """None where the format of that width refuses the values; else (sub, left, the constants' bits, the frame's samples per shape)."""
    if sub not in SUBS or siting not in SITINGS or matrix not in MATRICES or range_ not in RANGES:
        return None
    if width == 8:
        if SUBS[sub] not in yuv_ref.SUBSAMPLINGS or MATRICES[matrix] not in yuv_ref.MATRICES:   # subsampling 2 (4:2:2), matrix 2 (BT.2020)
            return None
        k = yuv_ref.Rule(MATRICES[matrix], RANGES[range_])
        k.mid = 128.0
        samples = [yuv_ref.frame_bytes(SUBS[sub], h, w) for h, w in SHAPES]
    else:
        if depth not in yuv16_ref.DEPTHS:
            return None
        k = yuv16_ref.Rule(MATRICES[matrix], RANGES[range_], depth)
        samples = [yuv16_ref.frame_samples(SUBS[sub], h, w) for h, w in SHAPES]
    k.ylo, k.yhi = k.ylim
    k.clo, k.chi = k.clim
    left = int(SUBS[sub] != "444" and SITINGS[siting] == "left")
    return sub, left, [bits(getattr(k, f)) for f in FIELDS], samples


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_rule_is_the_two_restatements(tmp_path, sanitize):
    """Every line the program prints (and once more under AddressSanitizer and UBSan: host code with its own main): the 16 combinations
    the 8-bit format accepts and the 20 it refuses for 4:2:2 or BT.2020; subsampling x siting x matrix x range x depth 9..16 of the deep
    format, depths 8 and 17 refused; an enum outside its values in each field refused by both."""
    res = subprocess.run([build(tmp_path, sanitize)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    seen = {8: [0, 0], 16: [0, 0]}   # [accepted, refused]
    for line in res.stdout.strip().split("\n"):
        tok = line.split()
        width, sub, siting, matrix, range_, depth = (int(t) for t in tok[:6])
        want = expected(width, sub, siting, matrix, range_, depth)
        if want is None:
            assert tok[6:] == ["refused"], line
            seen[width][1] += 1
            continue
        assert tok[6] == "ok" and tok[27] == ":" and len(tok) == 28 + len(SHAPES), line
        got = (int(tok[7]), int(tok[8]), [bits(float.fromhex(t)) for t in tok[9:27]], [int(t) for t in tok[28:]])
        assert got[:2] == want[:2], line
        for f, g, w in zip(FIELDS, got[2], want[2]):
            assert g == w, (line, f)
        assert got[3] == want[3], line
        seen[width][0] += 1
    assert seen[8] == [16, 36 - 16 + 8] and seen[16] == [3 * 2 * 3 * 2 * 8, 3 * 2 * 3 * 2 * 2 + 8], seen


def test_an_8_bit_format_is_the_deep_rule_at_depth_8():
    """What lets one maker serve both: yuv16_ref's constants, formed by its own operations at d = 8 (outside its DEPTHS), are yuv_ref's."""
    for matrix in yuv_ref.MATRICES:
        for range_ in yuv_ref.RANGES:
            a = yuv_ref.Rule(matrix, range_)
            b = yuv16_ref.Rule.__new__(yuv16_ref.Rule)
            depths, yuv16_ref.DEPTHS = yuv16_ref.DEPTHS, (8,)
            try:
                b.__init__(matrix, range_, 8)
            finally:
                yuv16_ref.DEPTHS = depths
            for f in ("kr", "kb", "kg", "cr2", "cb2", "ir", "ib", "ig", "oy", "sy", "sc", "ky", "kc"):
                assert bits(getattr(a, f)) == bits(getattr(b, f)), (matrix, range_, f)
            assert bits(b.mid) == bits(128.0) and tuple(map(bits, a.ylim + a.clim)) == tuple(map(bits, b.ylim + b.clim))
