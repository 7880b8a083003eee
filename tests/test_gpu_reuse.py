"""The row reuse of the frame stream on the GPU (include/srhip.h sr_video_set_reuse): the row-compare kernel against numpy at every
pointer offset, the session with the mode on against the session with it off and against the synchronous call, byte for byte, with the
counts the restatement (tests/reuse_ref.py) predicts; the whole-or-nothing paths, the split-half domain flag, refusals, lifetime, the CLI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reuse_ref
import yuv16_ref
import yuv_ref
from conftest import synth_u8

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "split_f16")
ROW_BYTES = (1, 15, 16, 17, 31, 33, 255, 4099)
ROWS = (1, 2, 5, 67)
# both pointers at every offset 0 .. 15; every offset of a against b at the same offset, one further (they share nothing), four
# further (4-byte path), seven and eight further
PAIRS = [(oa, (oa + k) % 16) for oa in range(16) for k in (0, 1, 4, 7, 8)]
SUB = {"420": reuse_ref.SUB_420, "444": reuse_ref.SUB_444, "422": reuse_ref.SUB_422}
# (name, subsampling, siting, depth): the 8-bit formats are BT.709 limited, the deep ones BT.709 limited at 10 bits
FORMATS = (("420center", "420", "center", 8), ("420left", "420", "left", 8), ("444", "444", "center", 8), ("420p10", "420", "left", 10),
           ("422p10", "422", "left", 10))
SIZES = ((64, 24), (63, 23))   # (rows, columns) of the LR frames: 24 x 64 and 23 x 63, the odd one for the chroma clamps


@pytest.fixture(scope="module")
def engines(params):
    import rusty_sr_amd as r
    from test_gpu_validation import synthetic_params
    made = {}

    def get(precision="f32", factor=3, graph="sr_net"):
        k = (precision, factor, graph)
        if k not in made:
            if graph != "sr_net":
                made[k] = r.Engine(graph=graph)
            else:
                made[k] = r.Engine(params["imagenet"] if factor == 3 else synthetic_params(factor, 100 + factor), device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------
def variants(rng, rows, rb):
    """a and seven b's of rows x rb bytes.  In b number v < 5 row r carries pattern (r + v) % 5: equal; the first, the last, a middle
    byte different; every byte different -- so that every row meets every pattern, a single row too.  Then all rows equal, all different."""
    a = rng.integers(0, 256, (rows, rb), dtype=np.uint8)
    out = []
    for v in range(5):
        b = a.copy()
        for r in range(rows):
            k = (r + v) % 5
            if k == 1:
                b[r, 0] ^= 0x01
            elif k == 2:
                b[r, rb - 1] ^= 0x80
            elif k == 3:
                b[r, rb // 2] ^= 0x10
            elif k == 4:
                b[r] ^= 0xFF
        out.append(b)
    out += [a.copy(), a ^ 0xFF]
    return a, out


@pytest.mark.parametrize("rb", ROW_BYTES)
def test_rows_differ_is_numpy_at_every_offset(engines, rb):
    """flags == (a != b).any(axis=1) for every row count, offset pair and pattern.  The bytes just before and just after the compared
    region differ between the two buffers (0x11 against 0xEE) and must not flag; the output starts as 0xFFFFFFFF words, so every flag
    has to be written; a second run gives the same words."""
    import torch
    e = engines()
    rng = np.random.default_rng(rb)
    pending = []
    for rows in ROWS:
        n = rows * rb
        a, bs = variants(rng, rows, rb)
        want = [(a != b).any(axis=1).astype(np.int32) for b in bs]
        assert want[5].sum() == 0 and want[6].sum() == rows and all(0 < w.sum() or rows < 2 for w in want[:5])
        a_dev = torch.from_numpy(a.reshape(-1)).cuda()
        b_dev = [torch.from_numpy(b.reshape(-1)).cuda() for b in bs]
        buf_a = torch.full((n + 48,), 0x11, dtype=torch.uint8, device="cuda")
        buf_b = torch.full((n + 48,), 0xEE, dtype=torch.uint8, device="cuda")
        assert buf_a.data_ptr() % 16 == 0 and buf_b.data_ptr() % 16 == 0
        for oa, ob in PAIRS:
            buf_a.fill_(0x11)
            va = buf_a[oa:oa + n]
            va.copy_(a_dev)
            for v, b in enumerate(b_dev):
                buf_b.fill_(0xEE)
                vb = buf_b[ob:ob + n]
                vb.copy_(b)
                out = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
                assert e.rows_differ_dev(va, vb, rows, rb, out=out) is out
                pending.append((out, want[v], (rows, oa, ob, v)))
                if v == 0:
                    pending.append((e.rows_differ_dev(va, vb, rows, rb), want[v], (rows, oa, ob, "again")))
    ops = e.last_plan()["ops"]
    assert len(ops) == 1 and ops[0]["name"] == "rows_differ" and ops[0]["bx"] == -(-ROWS[-1] // 4), ops
    torch.cuda.synchronize()
    got = torch.stack([torch.nn.functional.pad(o, (0, ROWS[-1] - o.numel())) for o, _, _ in pending]).cpu().numpy()
    for row, (_, want_flags, what) in zip(got, pending):
        assert row[:len(want_flags)].tolist() == want_flags.tolist(), (rb, what)


def test_rows_differ_past_the_grid_and_refusals(engines):
    """More rows than the grid has waves (64 x 256 workgroups of four): the waves take further rows a grid apart.  And what is refused."""
    import torch
    from rusty_sr_amd import _lib
    e = engines()
    rows, rb = 64 * 256 * 4 + 37, 3
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (rows, rb), dtype=np.uint8)
    b = a.copy()
    dirty = rng.random(rows) < 0.3
    dirty[[0, rows - 1, 64 * 256 * 4]] = True
    b[dirty, rng.integers(0, rb, int(dirty.sum()))] ^= 0x40
    whole_a, whole_b = torch.from_numpy(np.concatenate([[0], a.reshape(-1)]).astype(np.uint8)).cuda(), torch.from_numpy(b.reshape(-1)).cuda()
    out = e.rows_differ_dev(whole_a[1:], whole_b, rows, rb)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == dirty.astype(np.int32).tolist()
    L, INV = e._L, _lib.SR_E_INVALID
    pa, pb, po = C.c_void_p(whole_a.data_ptr()), C.c_void_p(whole_b.data_ptr()), C.c_void_p(out.data_ptr())
    before = out.clone()
    assert L.sr_rows_differ_dev(e._ctx, None, pb, 4, 3, po, None) == INV and L.sr_rows_differ_dev(e._ctx, pa, None, 4, 3, po, None) == INV
    assert L.sr_rows_differ_dev(e._ctx, pa, pb, 4, 3, None, None) == INV
    assert L.sr_rows_differ_dev(e._ctx, pa, pb, 0, 3, po, None) == INV and L.sr_rows_differ_dev(e._ctx, pa, pb, 4, 0, po, None) == INV
    assert L.sr_rows_differ_dev(e._ctx, pa, pb, 2 ** 31, 3, po, None) == INV and L.sr_rows_differ_dev(e._ctx, pa, pb, 4, 2 ** 63, po, None) == INV
    for off in (1, 2, 3):
        assert L.sr_rows_differ_dev(e._ctx, pa, pb, 4, 3, C.c_void_p(out.data_ptr() + off), None) == INV
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ---- 2. the session ----------------------------------------------------------------------------------------------------------------------
def make_format(sub, siting, depth):
    from rusty_sr_amd import Yuv16Format, YuvFormat
    return YuvFormat.named(sub, siting, "bt709", "limited") if depth == 8 else Yuv16Format.named(sub, siting, "bt709", "limited", depth)


def key_frame(seed, sub, siting, depth, h, w, dim=1):
    """A smooth picture as one frame of samples (u8, or u16 for a deep format); dim: its RGB divided by this."""
    x = (synth_u8(seed, 1, h, w)[0] // dim).astype(np.float32) / np.float32(255.0)
    if depth == 8:
        return yuv_ref.rgb_to_yuv(x, sub, siting, "bt709", "limited")
    return yuv16_ref.rgb_to_yuv(x, sub, siting, "bt709", "limited", depth)


def sequence(key, sub, h, w):
    """The nine frames: a key frame, the same again, one luma sample changed in row 30, one Cb sample changed (chroma row 10), a change
    in row 0, in row h - 1, in rows 4 and 58 together, in every row, and that frame again.  Each frame is the one before it with its change."""
    cw = w if sub == "444" else (w + 1) // 2
    steps = [[], [], [30 * w + 5], [h * w + 10 * cw + 3], [2], [(h - 1) * w + w - 1], [4 * w + 1, 58 * w + 7], [y * w + (y % w) for y in range(h)], []]
    frames, cur = [], key
    for change in steps:
        cur = cur.copy()
        cur[np.array(change, dtype=np.intp)] ^= 8
        frames.append(cur)
    return frames


def predicted(frames, sub, h, w, depth, whole_or_nothing=False):
    """What each frame adds to the session's counts: the first frame is whole; then the restatement's plan for the rows that differ."""
    out = []
    for i, f in enumerate(frames):
        plan = [(0, h)]
        if i:
            plan = reuse_ref.plan(reuse_ref.frame_flags(frames[i - 1], f, SUB[sub], h, w, 1 if depth == 8 else 2), SUB[sub], h)
            if whole_or_nothing:
                plan = reuse_ref.whole_or_nothing(plan, h)
        out.append(reuse_ref.frame_stats(plan, h))
    return out


def run(e, fmt, h, w, frames, slots, reuse, members=None, groups=None):
    """The frames through a session, the ring kept full (or, with groups, each group submitted whole and then received whole): the
    frames received and the session's counts after each submit."""
    import rusty_sr_amd as r
    v = r.VideoStream(e, fmt, h, w, slots=slots, members=members, reuse=reuse)
    got, stats = [], []
    if groups is None:
        for f in frames:
            if v.pending == slots:
                got.append(v.receive())
            v.submit(f)
            stats.append(v.reuse_stats())
        while v.pending:
            got.append(v.receive())
    else:
        for g in groups:
            for i in g:
                v.submit(frames[i])
                stats.append(v.reuse_stats())
            got += [v.receive() for _ in g]
    v.close()
    return got, stats


def deltas(stats):
    zero = dict.fromkeys(stats[0], 0)
    return [{k: b[k] - a[k] for k in b} for a, b in zip([zero] + stats[:-1], stats)]


def synchronous(e, fmt, h, w, frames, depth, members=1):
    call = e.upscale_yuv if depth == 8 else e.upscale_yuv16
    return [call(f, fmt, h, w, members).view(np.uint8).tobytes() for f in frames]


def check_sessions(e, name, sub, siting, depth, h, w, slots_list=(1, 3), members=None, whole_or_nothing=False):
    fmt = make_format(sub, siting, depth)
    frames = sequence(key_frame(700 + h, sub, siting, depth, h, w), sub, h, w)
    want = synchronous(e, fmt, h, w, frames, depth, 1 if members is None else members)   # once, for every slot count
    assert want[0] == want[1] and want[7] == want[8] and len(set(want)) == 7
    pred = predicted(frames, sub, h, w, depth, whole_or_nothing)
    if not whole_or_nothing:  # the sequence is what it claims: whole, reused, five partial frames (the seventh of two bands), whole, reused
        assert [(p["frames_full"], p["frames_reused"], p["frames_partial"], p["bands"]) for p in pred] == \
            [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 1, 1), (0, 0, 1, 2), (1, 0, 0, 0), (0, 1, 0, 0)], pred
    for slots in slots_list:
        off, off_stats = run(e, fmt, h, w, frames, slots, False, members)
        on, on_stats = run(e, fmt, h, w, frames, slots, True, members)
        assert all(v == 0 for s in off_stats for v in s.values())
        for i in range(len(frames)):
            assert off[i].tobytes() == want[i], (name, h, w, slots, i, "the stream as it is")
            assert on[i].tobytes() == want[i], (name, h, w, slots, i, "reuse")
        assert deltas(on_stats) == pred, (name, h, w, slots, deltas(on_stats), pred)
        total = on_stats[-1]
        assert total["frames"] == 9 and total["rows_total"] == 9 * h
        if whole_or_nothing:
            assert total["frames_partial"] == 0 and total["frames_reused"] == 2 and total["rows_computed"] == 7 * h
        else:
            assert total["rows_computed"] < total["rows_total"] and total["frames_partial"] == 5 and total["frames_reused"] == 2


@pytest.mark.parametrize("form", FORMATS, ids=[f[0] for f in FORMATS])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reuse_gives_the_streams_frames(engines, precision, form):
    name, sub, siting, depth = form
    for h, w in SIZES:
        check_sessions(engines(precision), name, sub, siting, depth, h, w)


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_reuse_at_factors_2_and_4(engines, precision, factor):
    check_sessions(engines(precision, factor), "420left", "420", "left", 8, 63, 23)


def test_whole_or_nothing_paths(engines):
    """An ensemble and the bilinear graph have no band form: a frame is reused whole or computed as with the mode off."""
    check_sessions(engines("f32"), "ensemble8", "420", "left", 8, 63, 23, slots_list=(3, ), members=0xFF, whole_or_nothing=True)
    check_sessions(engines(graph="bilinear"), "bilinear", "420", "center", 8, 63, 23, whole_or_nothing=True)


def test_reuse_with_a_frame_that_leaves_the_split_domain():
    """tests/domain_cases.py's wiring with channel 5 of the first layer = 2 (1.5e4 + 4e4 R) (every weight inside the domain), read by nothing: a
    dark picture (R <= 0.14: 4.1e4 on the f64 oracle) stays inside the split-half mode's domain, a white block leaves it (1.1e5 >= 65504).  The fourth frame
    has the block.  One slot, and three slots with
    the fourth, fifth (the same frame: reused whole) and sixth frame in flight together: the frames received are those of the session
    with the mode off under the same submissions -- split-half results before the fourth frame, exact f32 from it on, the frames after
    it reusing rows of f32 outputs -- and the context ends in exact f32."""
    import torch
    import domain_cases
    import grad_ref
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    h, w = 64, 24
    fmt = make_format("420", "left", 8)
    p = domain_cases.wired("f", 5, 4e4)
    off, n, shape = grad_ref.segments(3)["f_bias"]
    p[off:off + n].reshape(shape)[5] = 1.5e4
    dark = key_frame(11, "420", "left", 8, h, w, dim=5)
    d1 = dark.copy()
    d1[30 * w + 5] ^= 1
    bright = d1.copy()
    bright[:h * w].reshape(h, w)[40:44, 8:12] = 235
    bright[h * w:].reshape(2, h // 2, w // 2)[:, 20:22, 4:6] = 128
    after = bright.copy()
    after[4 * w + 1] ^= 1
    later = after.copy()
    later[50 * w + 2] ^= 1
    frames = [dark, dark, d1, bright, bright, after, after, later]
    probe = r.Engine(p, precision="split_f16")   # the premise
    for f, status in ((dark, _lib.SR_OK), (d1, _lib.SR_OK), (bright, _lib.SR_E_DOMAIN)):
        probe.upscale_yuv_dev(torch.from_numpy(f[None]).cuda(), fmt, h, w)
        torch.cuda.synchronize()
        assert probe._L.sr_check_domain(probe._ctx) == status
    probe.close()
    exact = r.Engine(p, precision="f32")
    want_f32 = synchronous(exact, fmt, h, w, frames, 8)
    exact.close()
    pred = predicted(frames, "420", h, w, 8)
    assert [q["frames_reused"] for q in pred] == [0, 1, 0, 0, 1, 0, 1, 0] and pred[3]["frames_partial"] == pred[5]["frames_partial"] == 1
    for slots, groups in ((1, [[i] for i in range(8)]), (3, [[0], [1], [2], [3, 4, 5], [6], [7]])):
        got = {}
        for reuse in (False, True):
            e = r.Engine(p, precision="split_f16")
            got[reuse], stats = run(e, fmt, h, w, frames, slots, reuse, groups=groups)
            if reuse:
                assert deltas(stats) == pred        # a frame queued again is not counted again
            e.check_domain()                         # the word was cleared
            e.upscale_yuv_dev(torch.from_numpy(bright[None]).cuda(), fmt, h, w)
            torch.cuda.synchronize()
            assert e._L.sr_check_domain(e._ctx) == _lib.SR_OK   # exact f32 now: the bright frame raises nothing
            e.close()
        for i in range(len(frames)):
            assert got[True][i].tobytes() == got[False][i].tobytes(), (slots, i)
            if i >= 3:
                assert got[True][i].tobytes() == want_f32[i], (slots, i)


def test_set_reuse_refusals_toggling_and_lifetime(params):
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    h, w = 63, 23
    fmt = make_format("420", "left", 8)
    frames = sequence(key_frame(5, "420", "left", 8, h, w), "420", h, w)
    e = r.Engine(params["imagenet"])
    want = synchronous(e, fmt, h, w, frames, 8)
    v = r.VideoStream(e, fmt, h, w, slots=3)
    L, INV = e._L, _lib.SR_E_INVALID
    for mode in (2, -1, 1 << 20):
        assert L.sr_video_set_reuse(v._v, mode) == INV
    assert L.sr_video_get_reuse_stats(v._v, None) == INV
    v.submit(frames[0])
    assert L.sr_video_set_reuse(v._v, 1) == INV and L.sr_video_set_reuse(v._v, 0) == INV   # a frame is pending
    assert v.receive().tobytes() == want[0] and v.reuse_stats()["frames"] == 0
    v.set_reuse(True)
    got = []
    for i in (1, 2, 3):                      # the first frame after the call is whole, although it is the frame before it again
        v.submit(frames[i])
        got.append(v.receive().tobytes())
    assert got == want[1:4] and v.reuse_stats()["frames_full"] == 1 and v.reuse_stats()["frames_partial"] == 2
    v.set_reuse(False)
    v.submit(frames[4])
    assert v.receive().tobytes() == want[4] and v.reuse_stats()["frames"] == 3
    v.set_reuse(_lib.SR_VIDEO_REUSE_ROWS)
    for i in (5, 6):
        v.submit(frames[i])
    assert [v.receive().tobytes() for _ in (5, 6)] == want[5:7]
    assert v.reuse_stats()["frames_full"] == 2 and v.reuse_stats()["frames_partial"] == 3
    for f in frames[6:9]:
        v.submit(f)
    v.close()                                # frames in flight: waits for them
    assert e.upscale_yuv(frames[0], fmt, h, w).tobytes() == want[0]
    v = r.VideoStream(e, fmt, h, w, slots=2, reuse=True)
    v.submit(frames[0])
    v.submit(frames[1])
    e.close()                                # the context goes first: the session is drained and detached
    assert v.pending == -1 and L.sr_video_set_reuse(v._v, 1) == INV
    assert L.sr_video_get_reuse_stats(v._v, C.byref(_lib.VideoReuseStats())) == INV
    v.close()


def test_a_change_of_precision_between_two_frames_makes_the_next_frame_whole(params):
    """Rows computed in one precision are not taken over into a frame of the other: the repeated frame is computed again (the counts
    show it; at 8 bits the two precisions' frames may well be the same bytes)."""
    import rusty_sr_amd as r
    h, w = 63, 23
    fmt = make_format("420", "left", 8)
    frame = key_frame(9, "420", "left", 8, h, w)
    e = r.Engine(params["imagenet"], precision="f32")
    want_f32 = e.upscale_yuv(frame, fmt, h, w).tobytes()
    v = r.VideoStream(e, fmt, h, w, slots=2, reuse=True)
    v.submit(frame)
    assert v.receive().tobytes() == want_f32
    e.set_precision("split_f16")
    want_split = e.upscale_yuv(frame, fmt, h, w).tobytes()
    v.submit(frame)
    assert v.receive().tobytes() == want_split
    v.submit(frame)
    assert v.receive().tobytes() == want_split
    st = v.reuse_stats()
    assert (st["frames_full"], st["frames_reused"], st["frames_partial"]) == (2, 1, 0)
    v.close()
    e.close()


def test_new_parameters_or_another_kernel_form_between_two_frames_make_the_next_frame_whole(params):
    """sr_set_params and the "wino" switch are legal while nothing is pending, and both change the bits a frame comes out with: the
    repeated frame after either is computed again, and the frame after that reuses rows of the new output.  Every frame is the frame of
    a session with the mode off that sees the same calls, and the synchronous call's under the parameters then in force."""
    import rusty_sr_amd as r
    h, w = 63, 23
    fmt = make_format("420", "left", 8)
    frame = key_frame(9, "420", "left", 8, h, w)
    changed = frame.copy()
    changed[30 * w + 5] ^= 8
    other = r.rsr.builtin("anime")
    got = {}
    for reuse in (False, True):
        e = r.Engine(params["imagenet"], precision="f32")
        v = r.VideoStream(e, fmt, h, w, slots=2, reuse=reuse)
        out, want = [], []

        def step(f):
            want.append(e.upscale_yuv(f, fmt, h, w).tobytes())   # (nothing is pending: the context takes the call)
            v.submit(f)
            out.append(v.receive().tobytes())

        step(frame)
        step(frame)
        e.set_params(other)
        step(frame)
        step(changed)
        e.set_experiment("wino", "0")
        step(changed)
        step(frame)
        assert out == want, [a == b for a, b in zip(out, want)]
        assert want[1] != want[2]                             # the premise: the two parameter sets differ on this frame
        if reuse:
            st = v.reuse_stats()
            assert (st["frames_full"], st["frames_reused"], st["frames_partial"]) == (3, 1, 2), st
        got[reuse] = out
        v.close()
        e.close()
    assert got[True] == got[False]


def test_partial_frames_launch_their_bands_only(engines):
    """What a frame queued, from the plan record and not from the session's own counts: the compare, the conversion to RGB of the whole
    frame, and for every band one pass of the conv stack whose last stage covers the band's rows (in whole tiles) and one conversion from
    RGB of exactly its 3 (y1 - y0) rows; a reused frame queues the compare alone, a whole frame the whole frame's launches."""
    import rusty_sr_amd as r
    e = engines("f32")
    h, w = SIZES[0]
    fmt = make_format("420", "left", 8)
    frames = sequence(key_frame(700 + h, "420", "left", 8, h, w), "420", h, w)
    v = r.VideoStream(e, fmt, h, w, slots=3, reuse=True)
    seen = []
    for i, f in enumerate(frames):
        v.submit(f)
        rec = e.last_plan()
        v.receive()
        bands = [(0, h)] if i == 0 else reuse_ref.plan(reuse_ref.frame_flags(frames[i - 1], f, SUB["420"], h, w), SUB["420"], h)
        ops = [(o["name"], o["by"]) for o in rec["ops"] for _ in range(o["count"])]
        last = [8 * l["ty8"] + 4 * l["ty4"] for l in rec["launches"] if l["st"] == 4 for _ in range(l["count"])]
        compare = [] if i == 0 else [("rows_differ", 1)]
        if not bands:
            assert ops == compare and rec["launches"] == [], (i, rec)
            continue
        assert ops == compare + [("yuv2rgb", -(-h // 2))] + [("rgb2yuv", -(-3 * (b - a) // 2)) for a, b in bands], (i, ops, bands)
        assert len(last) == len(bands) and all(b - a <= rows < b - a + 8 for (a, b), rows in zip(bands, last)), (i, last, bands)
        assert len([l for l in rec["launches"] for _ in range(l["count"])]) == 5 * len(bands), (i, rec["launches"])
        seen.append(sum(last))
    v.close()
    assert len(seen) == 7 and max(seen[1:6]) < h / 2 and seen[0] >= h and seen[6] >= h   # the five partial frames: less than half a frame each


# ---- 3. the CLI --------------------------------------------------------------------------------------------------------------------------
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rusty_sr_amd", "bin", "rusty_sr")


@pytest.mark.parametrize("deep", [False, True], ids=["8bit", "depth_auto"])
def test_cli_video_reuse(deep):
    from rusty_sr_amd.build import build_host
    from test_yuv_cpu import y4m_bytes
    build_host()
    h, w = 63, 23
    depth = 10 if deep else 8
    frames = sequence(key_frame(77, "420", "left", depth, h, w), "420", h, w)
    stream = y4m_bytes(f"YUV4MPEG2 W{w} H{h} F25:1 Ip {'C420p10' if deep else 'C420mpeg2'}", [f.tobytes() for f in frames])
    args = ["--depth", "auto"] if deep else []
    plain = subprocess.run([CLI, "video", *args, "--timing", "-", "-"], input=stream, capture_output=True, timeout=120)
    reuse = subprocess.run([CLI, "video", *args, "--reuse", "--timing", "-", "-"], input=stream, capture_output=True, timeout=120)
    assert plain.returncode == 0 and reuse.returncode == 0, (plain.stderr, reuse.stderr)
    out_bytes = (3 * h * 3 * w + 2 * ((3 * h + 1) // 2) * ((3 * w + 1) // 2)) * (2 if deep else 1)
    assert reuse.stdout == plain.stdout and len(plain.stdout) > 9 * out_bytes
    assert b"reuse" not in plain.stderr
    m = re.search(rb"\[timing\] reuse: (\d+) frames whole, (\d+) partial, (\d+) reused, (\d+\.\d) % of rows computed\n", reuse.stderr)
    assert m, reuse.stderr
    pred = predicted(frames, "420", h, w, depth)
    rows = sum(p["rows_computed"] for p in pred)
    assert [int(m.group(i)) for i in (1, 2, 3)] == [2, 5, 2] and m.group(4).decode() == f"{100.0 * rows / (9 * h):.1f}"
