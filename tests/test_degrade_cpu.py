"""The degradation operator's numpy restatement (tests/degrade_ref.py) held to everything it can be held to without a GPU: its own rounding
rule (the bytes do not depend on the arithmetic), the condition that lets the GPU test demand exact bytes, the oracle's pool, the 8
members, the noise stream's moments, Pillow's JPEG codec, and the --degrade spec and draw rule against the product's Python twin."""
import io
import math

import numpy as np
import pytest

import degrade_cases
import degrade_ref as ref
import oracle
from conftest import load_png

CASES = degrade_cases.cases()


def _img(case):
    return degrade_cases.image(*case["img"])


@pytest.fixture(scope="module")
def traced():
    """Every fixture case evaluated once in f64: name -> (bytes, trace)."""
    out = {}
    for c in CASES:
        trace = {}
        out[c["name"]] = (ref.degrade(_img(c), c["factor"], trace=trace, **degrade_cases.params(c)), trace)
    return out


def test_case_names_are_unique_and_cover_the_issue():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert {c["factor"] for c in CASES} == {2, 3, 4} and {c["member"] for c in CASES} == set(range(8))
    assert {0.0, 0.3, 1.7, 4.0} <= {c["sigma"] for c in CASES} and {0, 1, 50, 100} <= {c["quality"] for c in CASES}
    assert {c["img"][4] for c in CASES} == {3, 4}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_bytes_do_not_depend_on_the_arithmetic(case, traced):
    """Rounding robustness: long double, and f64 with every sum taken in the opposite order, give the f64 bytes."""
    want = traced[case["name"]][0]
    for ar in (ref.LONGDOUBLE, ref.REASSOCIATED):
        got = ref.degrade(_img(case), case["factor"], ar=ar, **degrade_cases.params(case))
        assert np.array_equal(got, want), (ar.name, int((got != want).sum()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_no_value_sits_at_a_rounding_boundary(case, traced):
    """The precondition of the GPU test's exact comparison: every value that is rounded lies at least 1e-11 from the point where its
    rounding changes (the structural ties sit at 2^-30 = 9.3e-10, by the rule's bias).  Two correct f64 evaluations differ by a few
    ulps of values below 2^11, i.e. by less than 1e-12."""
    _, trace = traced[case["name"]]
    assert "pixel" in trace
    for site, parts in trace.items():
        d = min(float(p.min()) for p in parts)
        assert d >= 1e-11, (site, d)


def test_bias_is_what_protects_the_ties():
    """Without blur and noise a JPEG block's DC and (0,4), (4,0), (4,4) coefficients are k / 8 over an integer table entry: exact ties
    occur (at quality 100, where the entries are 1, in one block out of eight), and they sit at 2^-30 to within the sums' rounding."""
    c = next(c for c in CASES if c["name"] == "jpeg-100")
    trace = {}
    ref.degrade(_img(c), c["factor"], trace=trace, **degrade_cases.params(c))
    d = np.concatenate(trace["quant"])
    assert np.any(np.abs(d - 2.0 ** -30) < 1e-11)


@pytest.mark.parametrize("seed,h,w", [(1, 24, 30), (2, 31, 28)])
def test_identity_case_is_the_rounded_pool_of_the_oracle(seed, h, w):
    """sigma = noise = quality = 0 at factor 3: the 8-bit quantisation of the pooled calls' input, LinearToSrgb(mean(SrgbToLinear))."""
    px = degrade_cases.image("smooth", seed, h, w)
    pooled = oracle.downsample(px.astype(np.float64) / 255.0, f64=True)[0]
    want = np.clip(np.floor(255.0 * pooled + 0.5 + ref.BIAS), 0, 255).astype(np.uint8)
    assert np.array_equal(ref.degrade(px, 3), want)


def _transform(a, k):
    if k & 4:
        a = a.transpose(1, 0, 2)
    if k & 2:
        a = a[::-1]
    if k & 1:
        a = a[:, ::-1]
    return a


@pytest.mark.parametrize("k", range(8))
def test_blur_and_pool_commute_with_the_members(k):
    """On a window whose blur stays inside the image, member k of the window degraded = T_k of the window degraded (no noise, no JPEG:
    the noise index and the block grid are anchored in the frame): byte for byte, although the sums run in another order."""
    px = degrade_cases.image("smooth", 70, 60, 64)
    fh, fw = 24, 36
    plain = ref.degrade(px, 3, sigma=1.7, window=(14, 13, fw, fh) if k & 4 else (14, 13, fh, fw))
    got = ref.degrade(px, 3, sigma=1.7, window=(14, 13, fh, fw), member=k)
    want = _transform(plain, k)
    assert got.shape == want.shape == (fh // 3, fw // 3, 3)
    assert np.array_equal(got, want)


def test_noise_stream_moments():
    """Mean and standard deviation of 64 x 64 x 3 values of the stream within 4 standard errors."""
    n = 64 * 64 * 3
    v = ref.noise_values(1.0, 12345, n)
    assert abs(v.mean()) < 4.0 / math.sqrt(n)
    assert abs(v.std() - 1.0) < 4.0 / math.sqrt(2 * n)
    assert np.array_equal(ref.noise_values(8.0, 12345, 16), np.float64(8.0) * ref.noise_values(1.0, 12345, 16))
    # random access: value i is outputs 2i + 1 and 2i + 2 of the sequential generator
    s, seq = 12345, []
    for _ in range(6):
        s = (s + ref.GOLDEN) & ref.MASK
        seq.append(ref.mix(s))
    assert seq == [ref.stream_output(12345, j) for j in range(1, 7)]


# Measured with this restatement (DESIGN.md 4o has the table): the largest mean absolute difference is PILLOW_WORST; the bar is twice it.
PILLOW_WORST = 0.716
PILLOW_IMAGES = [("butterfly_lr.png", None), ("cartoon_lr.png", None), ("logo_nn.png", None), ("butterfly_lr.png", (13, 10)),
                 ("cartoon_lr.png", (13, 10)), ("logo_nn.png", (13, 10))]


def pillow_difference(name, cut, q):
    from PIL import Image
    px = load_png(name)[..., :3]
    if cut:
        px = px[5:5 + cut[0], 7:7 + cut[1]]
    px = np.ascontiguousarray(px)
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="JPEG", quality=q, subsampling=0)
    theirs = np.array(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).astype(np.float64)
    ours = ref.jpeg_round_trip(px.astype(np.float64), q)
    return float(np.abs(ours - theirs).mean())


@pytest.mark.parametrize("q", [10, 40, 75, 95])
@pytest.mark.parametrize("name,cut", PILLOW_IMAGES)
def test_jpeg_stage_against_pillow(name, cut, q):
    """The same model (tables, 4:4:4, colour matrices), another decoder's arithmetic (integer DCT, fixed-point colour)."""
    pytest.importorskip("PIL")
    assert pillow_difference(name, cut, q) <= 2.0 * PILLOW_WORST


def test_spec_parsing_and_refusals():
    import rusty_sr_amd as r
    for parse in (ref.parse_spec, r.parse_degrade_spec):
        assert parse("blur=0.5:2,noise=0:8,jpeg=30:90") == {"blur": (0.5, 2.0), "noise": (0.0, 8.0), "jpeg": (30, 90)}
        assert parse("jpeg=75") == {"blur": (0.0, 0.0), "noise": (0.0, 0.0), "jpeg": (75, 75)}
        assert parse("noise=3,blur=4") == {"blur": (4.0, 4.0), "noise": (3.0, 3.0), "jpeg": (0, 0)}
        for bad, key in (("", ""), ("blurr=1", "blurr"), ("blur", "blur"), ("blur=1,blur=2", "blur"), ("blur=a", "blur"), ("blur=1:2:3", "blur"),
                         ("blur=2:1", "blur"), ("blur=0:4.5", "blur"), ("blur=-1:2", "blur"), ("noise=0:65", "noise"), ("noise=nan", "noise"),
                         ("jpeg=90:30", "jpeg"), ("jpeg=0:101", "jpeg"), ("jpeg=7.5", "jpeg"), ("blur=1,,jpeg=3", ""), ("blur=1,jpeg=", "jpeg")):
            with pytest.raises(ValueError) as e:
                parse(bad)
            assert f"'{key}'" in str(e.value) or not key, (bad, str(e.value))


def test_draw_stream():
    import rusty_sr_amd as r
    spec = ref.parse_spec("blur=0.5:2,noise=0:8,jpeg=30:90")
    a, b = ref.draws(spec, 7, 5), r.degrade_draws("blur=0.5:2,noise=0:8,jpeg=30:90", 7, 5)
    assert a == b
    assert r.degrade_draws(spec, 7, 2, first=3) == a[3:]
    for d in a:
        assert 0.5 <= d["sigma"] < 2 and 0 <= d["noise"] < 8 and 30 <= d["quality"] <= 90 and 0 <= d["seed"] < 2 ** 64
    # four outputs of the stream seeded with seed ^ 0xD6E8FEB86659FD93 per draw; the fourth is the noise seed as is
    s = 7 ^ 0xD6E8FEB86659FD93
    assert a[1]["seed"] == ref.stream_output(s, 8) and a[0]["sigma"] == 0.5 + ref.uniform(ref.stream_output(s, 1)) * 1.5
    many = ref.draws(ref.parse_spec("jpeg=1:4"), 3, 400)
    assert {d["quality"] for d in many} == {1, 2, 3, 4} and all(d["sigma"] == 0 and d["noise"] == 0 for d in many)
    assert ref.draws(spec, 8, 3) != a[:3]


def _asan(*args):
    """the sanitized stand-alone program (AddressSanitizer + UBSan, its own main) that links the CLI's spec parser and draw stream"""
    import subprocess
    from rusty_sr_amd.build import build_sanitized
    return subprocess.run([build_sanitized(), "--degrade-spec", *args], capture_output=True, text=True, timeout=120)


def test_cli_parser_and_draws_under_sanitizers_equal_the_python_twin():
    spec = "blur=0.5:2,noise=0:8,jpeg=30:90"
    for text, seed in ((spec, 7), ("jpeg=1:100", 2 ** 64 - 1), ("noise=64,blur=4", 0), ("blur=1e-1:.5e1", 3)):
        if text.startswith("blur=1e-1"):
            res = _asan(text, str(seed), "1")
            assert res.returncode == 1 and "'blur'" in res.stdout and not res.stderr  # .5e1 = 5 > 4
            continue
        res = _asan(text, str(seed), "9")
        assert res.returncode == 0 and not res.stderr, res.stderr
        want = ["%08x %08x %d %d" % (np.float32(d["sigma"]).view(np.uint32), np.float32(d["noise"]).view(np.uint32), d["quality"], d["seed"])
                for d in ref.draws(ref.parse_spec(text), seed, 9)]
        assert res.stdout.splitlines() == want
    for bad, key in (("blurr=1", "blurr"), ("blur", "blur"), ("blur=1,blur=2", "blur"), ("blur=a", "blur"), ("blur=1:2:3", "blur"),
                     ("blur=2:1", "blur"), ("blur=0:4.5", "blur"), ("blur=-1:2", "blur"), ("noise=0:65", "noise"), ("noise=nan", "noise"),
                     ("noise=inf", "noise"), ("noise=0x10", "noise"), ("noise= 1", "noise"), ("jpeg=90:30", "jpeg"), ("jpeg=0:101", "jpeg"),
                     ("jpeg=7.5", "jpeg"), ("blur=1,,jpeg=3", ""), ("blur=1,jpeg=", "jpeg"), ("blur=" + "9" * 400, "blur"), ("", "")):
        res = _asan(bad, "1", "1")
        assert res.returncode == 1 and res.stdout.startswith("error: ") and f"'{key}'" in res.stdout + "''" and not res.stderr, (bad, res.stdout, res.stderr)
        with pytest.raises(ValueError):
            ref.parse_spec(bad)


def test_cli_refuses_bad_specs_by_name_before_it_needs_a_device(tmp_path):
    import subprocess
    from rusty_sr_amd.build import build_host
    cli = build_host()
    run = lambda *a: subprocess.run([cli, *a], capture_output=True, text=True, timeout=120)
    for sub, tail in (("train", [str(tmp_path / "p.rsr"), str(tmp_path)]), ("validate", [str(tmp_path)])):
        for bad, key in (("blur=2:1", "blur"), ("noise=0:65", "noise"), ("jpeg=x", "jpeg"), ("sharpen=1", "sharpen")):
            res = run(sub, "--degrade", bad, *tail)
            assert res.returncode == 2 and f"'{key}'" in res.stderr and "--degrade <SPEC>" in res.stderr, res.stderr
        res = run(sub, "--degrade", "blur=1", "--lr_folder", str(tmp_path), *tail)
        assert res.returncode == 2 and "'--degrade <SPEC>' cannot be used with '--lr_folder <DIR>'" in res.stderr, res.stderr
        res = run(sub, "--degrade")
        assert res.returncode == 2 and "requires a value" in res.stderr
    res = run("train", "--degrade", "blur=1", "-v", str(tmp_path), "--val_lr_folder", str(tmp_path), str(tmp_path / "p.rsr"), str(tmp_path))
    assert res.returncode == 2 and "'--val_lr_folder <DIR>'" in res.stderr
    res = run("validate", "--seed", "3", str(tmp_path))
    assert res.returncode == 2 and "--degrade <SPEC>" in res.stderr
    res = run("--degrade", "blur=1", "a.png", "b.png")
    assert res.returncode == 2 and "'train' and 'validate'" in res.stderr
    for sub in ("train", "validate"):
        assert "--degrade <SPEC>" in run(sub, "--help").stdout
