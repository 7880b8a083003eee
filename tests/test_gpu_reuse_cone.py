"""The row reuse of the frame stream at the edge of its dependency cone (the cases and their premises: tests/reuse_cases.py,
tests/test_reuse_cases_cpu.py).  tests/test_gpu_reuse.py changes one sample of a smooth 8- or 10-bit picture by 8: that reaches neither
the outer row of the planner's margin nor the outer halo row of a band, and its frames are too short for three bands.  Here a changed row
is a black / white checker, the formats go to 16 bits full range, and the frames are tall enough for every plan the planner can make.

Every list of frames is held to three things, in this order.  The WITNESS, on the synchronous call's frames (the mode off: not the code
under test): between a frame and the one before it the first and the last LR row of every band's cone differ in the output -- without it
the byte comparison could turn weak unnoticed when weights or pictures change.  Then the frames with reuse on, with reuse off and of the
synchronous call agree byte for byte.  Then the counts are the restatement's."""
import numpy as np
import pytest

import reuse_cases as rc
import reuse_ref
from test_gpu_reuse import PRECISIONS, deltas, engines, make_format, predicted, run, synchronous  # noqa: F401 (engines: a fixture)

pytestmark = pytest.mark.gpu

DEEP_OPS = {8: "rgb2yuv", 10: "rgb_to_yuv16", 16: "rgb_to_yuv16"}


def fmt_of(name):
    """make_format of tests/test_gpu_reuse.py, extended by the range and by depth 16."""
    from rusty_sr_amd import Yuv16Format
    sub, siting, rng, depth = rc.FORMATS[name]
    return make_format(sub, siting, depth) if rng == "limited" else Yuv16Format.named(sub, siting, "bt709", rng, depth)


def check(e, name, h, w, frames, slots_list=(1, 3), groups=None, plans=None, no_witness=()):
    """The three checks of the module's docstring for one list of frames; groups: how slots = 3 submits them (slots = 1 keeps the ring
    full, one frame); plans: the literal plans of the frames after the first; no_witness: the (frame, band, "top" | "bottom") a weight
    set is known not to carry a change to (the caller prints them); every other side of every band is required.  Returns the witness rows."""
    sub, _, _, depth = rc.FORMATS[name]
    f, fmt = e.factor, fmt_of(name)
    want = synchronous(e, fmt, h, w, frames, depth)   # once, for every slot count
    dtype = np.uint8 if depth == 8 else np.uint16
    seen = rc.witness([np.frombuffer(b, dtype=dtype) for b in want], frames, name, h, w, f)
    assert seen, ("witness lost", name, h, w)
    for i, band, top, bottom in seen:
        for side, count in (("top", top), ("bottom", bottom)):
            assert count > 0 or (i, band, side) in no_witness, ("witness lost", name, h, w, f, i, band, side, seen)
    pred = predicted(frames, sub, h, w, depth)
    for slots in slots_list:
        g = groups if slots > 1 else None
        off, off_stats = run(e, fmt, h, w, frames, slots, False, groups=g)
        on, on_stats = run(e, fmt, h, w, frames, slots, True, groups=g)
        for i in range(len(frames)):
            assert off[i].tobytes() == want[i], (name, h, w, slots, i, "the stream as it is")
            if on[i].tobytes() != want[i]:
                rows = [np.flatnonzero((p != q).any(axis=1)).tolist() for p, q in
                        zip(rc.planes(on[i].view(dtype), name, f * h, f * w), rc.planes(np.frombuffer(want[i], dtype=dtype), name, f * h, f * w))]
                where = ", ".join(f"{p} {r[0]}..{r[-1]} ({len(r)})" for p, r in zip(("Y", "Cb", "Cr"), rows) if r)
                pytest.fail(f"{name} {h} x {w}, {slots} slot(s), frame {i}: reuse gives other bytes, in output rows {where}", pytrace=False)
        assert all(v == 0 for s in off_stats for v in s.values())
        assert deltas(on_stats) == pred, (name, h, w, slots, deltas(on_stats), pred)
        total = on_stats[-1]
        assert total["frames"] == len(frames) and total["rows_total"] == len(frames) * h
        assert total["rows_computed"] == sum(p["rows_computed"] for p in pred) < total["rows_total"]
    if plans is not None:   # ... and the counts are those of the plans the case names
        assert pred[1:] == [reuse_ref.frame_stats(p, h) for p in plans], (name, h, w)
    # the context is still in its mode (a frame that leaves the split-half domain would have left it in exact f32, for good)
    synchronous(e, fmt, h, w, frames[:1], depth)
    launches = e.last_plan()["launches"]
    assert launches and all(l["prec"] == e.precision for l in launches), launches
    return seen


@pytest.mark.parametrize("name", list(rc.FORMATS))
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h,w,mid", [(64, 24, 30), (160, 40, 80)])
def test_cone_edge_is_recomputed(engines, h, w, mid, precision, name):
    """One checker row in the interior, one at row 15 (band (8, 24): the top halo begins at input row 1) and one at row h - 16 (the
    mirror case).  An even row's cone begins one row below its band's even edge, an odd row's ends one row above: a planner margin of
    6 loses that row on the one side or the other."""
    changes = [[rc.checker(mid)], [rc.checker(15)], [rc.checker(h - 16)]]
    plans = [[(mid - 8, mid + 8)], [(8, 24)], [(h - 24, h - 8)]]
    frames = rc.build(rc.key_frame("smooth", name, h, w), changes, name, h, w)
    check(engines(precision), name, h, w, frames, plans=plans)


@pytest.mark.parametrize("name", ["444p16", "420p16"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_band_halo_is_the_pictures_rows(params, precision, name):
    """A noise key frame at 16 bits, full range, where one halo row too few costs a hundred levels (tests/test_reuse_cases_cpu.py):
    the bands (8, 24), (136, 152) and an interior one.  In split-half the frames must be that mode's results and not the exact
    recompute, so the premise -- no frame leaves the mode's domain -- is held on a probe engine first."""
    import torch
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    h, w = 160, 40
    changes = [[rc.checker(15)], [rc.checker(144)], [rc.checker(80)]]
    frames = rc.build(rc.key_frame("noise", name, h, w), changes, name, h, w)
    fmt = fmt_of(name)
    if precision == "split_f16":
        probe = r.Engine(params["imagenet"], precision=precision)
        for fr in frames:
            probe.upscale_yuv16_dev(torch.from_numpy(fr.view(np.int16)[None]).cuda(), fmt, h, w)
            torch.cuda.synchronize()
            assert probe._L.sr_check_domain(probe._ctx) == _lib.SR_OK, "the premise: pick another noise seed"
        probe.close()
    e = r.Engine(params["imagenet"], precision=precision)
    try:
        check(e, name, h, w, frames, plans=[[(8, 24)], [(136, 152)], [(72, 88)]])
        e.check_domain()
    finally:
        e.close()


@pytest.mark.parametrize("name", ["420left", "444p16", "420p10"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h,w", [(160, 40), (161, 39)])
def test_three_and_four_bands_and_the_merge(engines, h, w, precision, name):
    """Every row of the sequence (tests/reuse_cases.py SEQUENCE): three and four bands, more runs than bands, the 13 / 14 row gap, the
    edge rules on both sides, the whole frame by cost, the 4:2:0 chroma rows.  With three slots the repeated frame and the four-band
    frame after it are in flight together."""
    labels, changes, plans = rc.sequence(name, h)
    frames = rc.build(rc.key_frame("smooth", name, h, w), changes, name, h, w)
    again = 1 + labels.index("the frame again")
    groups = [[i] for i in range(again)] + [[again, again + 1]] + [[i] for i in range(again + 2, len(frames))]
    check(engines(precision), name, h, w, frames, groups=groups, plans=plans)


@pytest.mark.parametrize("name", ["420left", "420p10"])
@pytest.mark.parametrize("factor,w", [(3, 344), (4, 260)])
def test_wide_frame(engines, factor, w, name):
    """A band wider than one SR_YUV_SPAN block of the conversion from RGB (3 x 344 = 1032, 4 x 260 = 1040 > 1024 output columns) and
    than the stage kernels' 32-column tiles, many times: the plan record shows the band's conversion with two column blocks."""
    import rusty_sr_amd as r
    from rusty_sr_amd import _lib
    assert factor * w > _lib.SR_YUV_SPAN >= factor * w // 2
    h, e = 40, engines("f32", factor)
    frames = rc.build(rc.key_frame("smooth", name, h, w), [[rc.checker(20)]], name, h, w)
    check(e, name, h, w, frames, slots_list=(3, ), plans=[[(12, 28)]])
    v = r.VideoStream(e, fmt_of(name), h, w, slots=3, reuse=True)
    v.submit(frames[0])
    v.receive()
    v.submit(frames[1])
    ops = [o for o in e.last_plan()["ops"] if o["name"] == DEEP_OPS[rc.FORMATS[name][3]]]
    v.receive()
    v.close()
    assert [(o["bx"], o["by"], o["count"]) for o in ops] == [(2, factor * 16 // 2, 1)], ops


# (frame, band, side) of test_factors_2_and_4 at factor 2: 0 samples of the cone's top row differ on synthetic_params(2, 102)
NO_WITNESS_F2 = ((1, (12, 28), "top"), (1, (132, 148), "top"), (3, (0, 18), "top"))


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_factors_2_and_4(engines, precision, factor):
    """The three-band frame, the frame again and the four-band frame at 160 x 40 on the synthetic weights of tests/test_gpu_reuse.py.
    The factor-4 set carries the checker to both outer rows of every cone: required, like everywhere else.  The factor-2 set does not
    carry it to the top row of three cones (NO_WITNESS_F2; nothing says an untrained weight set carries a change 7 rows, and the weights
    are not tuned for it): printed there, and the other eleven sides are required."""
    name, h, w = "420left", 160, 40
    labels, changes, plans = rc.sequence(name, h)
    frames = rc.build(rc.key_frame("smooth", name, h, w), changes[:3], name, h, w)
    seen = check(engines(precision, factor), name, h, w, frames, groups=[[0], [1], [2, 3]], plans=plans[:3],
                 no_witness=NO_WITNESS_F2 if factor == 2 else ())
    print(f"\n  factor {factor}, {precision}: luma samples that differ in the cone's first / last LR row, of {factor * factor * w}, per band:")
    for i, band, top, bottom in seen:
        print(f"    frame {i} band {band}: {top} / {bottom}{'' if top and bottom else '   (no witness)'}")
