"""The premises of tests/test_gpu_reuse_cone.py, held on the references alone (tests/reuse_cases.py, tests/reuse_ref.py, the CPU oracle,
the colour restatements): the sequences' plans are the literal band lists; a checker row changes every output row of its 15-row cone
in every format, where the old tests' one-sample change leaves the cone's outer rows as they were at 8 bits; a band cut with one halo
row too few differs from the whole frame in a deep format, and with SR_HALO rows it does not.  These are conditions on the inputs, not
measurements of the library: if a seed fails one, change the seed, not the condition."""
import numpy as np
import pytest

import oracle
import reuse_cases as rc
import reuse_ref

F = 3
HALO = reuse_ref.SR_HALO


@pytest.fixture(scope="module")
def upscaled(params):
    """frame -> the frame the pipeline gives for it, by the references: restatement to RGB, the f32 oracle, restatement back."""
    def up(frame, name, h, w):
        return rc.to_frame(oracle.forward_factor(params["imagenet"], rc.to_rgb(frame, name, h, w), F)[0], name)
    return up


def test_the_cases_cover_the_issue():
    assert set(rc.FORMATS) == {"420left", "444", "420p10", "444p16", "420p16"} and rc.FORMATS["444p16"][2:] == ("full", 16)
    assert 3 * 344 > 1024 and 4 * 260 > 1024     # SR_YUV_SPAN (rusty_sr_amd/_lib.py; not imported: this file needs no library)
    labels, changes, plans = rc.sequence("420left", 160)
    assert sorted(len(p) for p in plans if p != [(0, 160)]) == [0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 4] and plans.count([(0, 160)]) == 1
    i = labels.index("the frame again")
    assert plans[i] == [] and len(plans[i + 1]) == 4      # the repeated frame directly before a multi-band frame


@pytest.mark.parametrize("name", list(rc.FORMATS))
@pytest.mark.parametrize("h,w", [(160, 40), (161, 39)])
def test_plans_are_the_literal_band_lists(name, h, w):
    labels, changes, plans = rc.sequence(name, h)
    frames = rc.build(rc.key_frame("smooth", name, h, w), changes, name, h, w)
    got = rc.plans_of(frames, name, h, w)
    for label, g, want in zip(labels, got, plans):
        assert g == want, (label, g, want)
    if (h, name) == (160, "420left"):
        print()
        for label, want in zip(labels, plans):
            print(f"  {label:62s} {want}")


def test_single_row_plans_at_the_other_sizes():
    """The rows of test_cone_edge_is_recomputed and test_wide_frame."""
    for (h, w), row, want in (((64, 24), 30, (22, 38)), ((64, 24), 15, (8, 24)), ((64, 24), 48, (40, 56)), ((160, 40), 80, (72, 88)),
                              ((160, 40), 15, (8, 24)), ((160, 40), 144, (136, 152)), ((40, 344), 20, (12, 28)), ((40, 260), 20, (12, 28))):
        for name in rc.FORMATS:
            key = rc.key_frame("smooth", name, h, w)
            assert rc.plans_of([key, rc.apply(key, rc.checker(row), name, h, w)], name, h, w) == [[want]], (h, w, row, name)
            assert rc.cones(key, rc.apply(key, rc.checker(row), name, h, w), name, h, w) == [(want, row - HALO, row + HALO)]


def differing(a, b, name, h, w):
    """Per output row, the number of luma samples that differ between two upscaled frames."""
    return (rc.planes(a, name, F * h, F * w)[0] != rc.planes(b, name, F * h, F * w)[0]).sum(axis=1)


@pytest.mark.parametrize("h,w,row", [(64, 24, 30), (160, 40, 80)])
def test_cone_witness(upscaled, h, w, row):
    """A checker in LR row r: every output row F (r - 7) .. F (r + 7) + F - 1 holds a differing luma sample, in every format, and none
    outside.  The old change (one sample ^= 8): at 8 bits the cone's outer LR row on either side is unchanged -- what a planner margin
    of 6 recomputes is all that differs, so no 8-bit frame of the old tests could tell 6 from 7."""
    lo, hi = F * (row - HALO), F * (row + HALO) + F
    print(f"\n  {h} x {w}, LR row {row}: differing luma samples in the cone's outer LR row (top / bottom), of {F * F * w} each")
    for name in rc.FORMATS:
        key = rc.key_frame("smooth", name, h, w)
        base = upscaled(key, name, h, w)
        counts = {}
        for change in (rc.checker(row), rc.tick(row)):
            d = differing(base, upscaled(rc.apply(key, change, name, h, w), name, h, w), name, h, w)
            assert d[:lo].sum() == 0 and d[hi:].sum() == 0, (name, change)
            counts[change[0]] = (d, int(d[lo:lo + F].sum()), int(d[hi - F:hi].sum()))
        print(f"  {name:8s} checker {counts['checker'][1]:4d} / {counts['checker'][2]:4d} (every row: >= {int(counts['checker'][0][lo:hi].min())})"
              f"   tick {counts['tick'][1]:4d} / {counts['tick'][2]:4d}")
        assert counts["checker"][0][lo:hi].min() >= 1, (name, "a cone row without a change")
        if rc.FORMATS[name][3] == 8:
            assert counts["tick"][1] == 0 and counts["tick"][2] == 0, (name, "the weak change reaches the cone's edge")
            assert counts["tick"][0].sum() > 0


@pytest.mark.parametrize("name", list(rc.FORMATS))
@pytest.mark.parametrize("h,w", [(160, 40), (161, 39)])
def test_sequence_witness(upscaled, h, w, name):
    """What the GPU test asserts on the synchronous frames, here on the oracle's: in every frame of the sequence the first and the last
    LR row of every band's cone differ from the frame before -- with the checkers of the earlier frames in the picture, for merged
    bands, at the image edges and for the chroma rows (the weakest: a changed chroma row reaches its outer two luma rows with a quarter
    of its weight, and at 8 bits a handful of samples of the cone's outer rows show it)."""
    labels, changes, _ = rc.sequence(name, h)
    frames = rc.build(rc.key_frame("smooth", name, h, w), changes, name, h, w)
    seen = rc.witness([upscaled(fr, name, h, w) for fr in frames], frames, name, h, w, F)
    assert len(seen) == sum(len(p) for p in rc.plans_of(frames, name, h, w) if p != [(0, h)])
    chroma = [min(s[2:]) for s in seen if labels[s[0] - 1].startswith("420:")]
    print(f"\n  {h} x {w} {name:8s} fewest differing samples in a cone's outer LR row, of {F * F * w}: checker rows "
          f"{min(min(s[2:]) for s in seen if not labels[s[0] - 1].startswith('420:'))}, chroma rows {min(chroma) if chroma else '-'}")
    assert all(top and bottom for _, _, top, bottom in seen), [s for s in seen if not (s[2] and s[3])]


@pytest.mark.parametrize("kind,name,h,w,rows", [("smooth", n, h, w, rows) for n in rc.FORMATS for h, w, rows in
                                                ((64, 24, (30, 15, 48)), (160, 40, (80, 15, 144)), (40, 344, (20, )))] +
                         [("noise", n, 160, 40, (15, 144, 80)) for n in ("444p16", "420p16")])
def test_single_row_witness(upscaled, kind, name, h, w, rows):
    """The same for the frames of test_cone_edge_is_recomputed, test_wide_frame and test_band_halo_is_the_pictures_rows."""
    frames = rc.build(rc.key_frame(kind, name, h, w), [[rc.checker(r)] for r in rows], name, h, w)
    seen = rc.witness([upscaled(fr, name, h, w) for fr in frames], frames, name, h, w, F)
    assert len(seen) == len(rows) and all(top and bottom for _, _, top, bottom in seen), seen


@pytest.mark.parametrize("y0,y1", [(8, 24), (72, 88), (136, 152)])
def test_halo_witness(params, y0, y1):
    """A band of the noise key frame computed from its rows and 6 halo rows on either side differs from the whole frame's samples in
    its first F and its last F output rows, in 444p16 full range; with SR_HALO rows it is the whole frame's band exactly."""
    h, w, name = 160, 40, "444p16"
    rgb = rc.to_rgb(rc.key_frame("noise", name, h, w), name, h, w)
    forward = lambda x: oracle.forward_factor(params["imagenet"], x, F)[0]
    whole = rc.planes(rc.to_frame(forward(rgb), name), name, F * h, F * w)[0][F * y0:F * y1].astype(np.int64)
    got = {}
    for halo in (HALO - 1, HALO):
        out = forward(rgb[y0 - halo:y1 + halo])[F * halo:F * (halo + y1 - y0)]
        got[halo] = rc.planes(rc.to_frame(out, name), name, F * (y1 - y0), F * w)[0].astype(np.int64)
    assert np.array_equal(got[HALO], whole)
    d = np.abs(got[HALO - 1] - whole)
    print(f"\n  band ({y0}, {y1}), 6 halo rows: largest luma difference in the first / last {F} output rows {d[:F].max()} / {d[-F:].max()} "
          f"of 65535 levels ({(d[:F] != 0).sum()} / {(d[-F:] != 0).sum()} samples of {F * F * w}); rows between: {d[F:-F].max()}")
    assert d[:F].max() > 0 and d[-F:].max() > 0 and d[F:-F].max() == 0
    # for the record (no condition): the same cut of the smooth key frame, in levels of the 8-bit limited-range luma (219 to the unit)
    name = "420left"
    rgb = rc.to_rgb(rc.key_frame("smooth", name, h, w), name, h, w)
    whole_f, cut_f = forward(rgb)[F * y0:F * y1], forward(rgb[y0 - HALO + 1:y1 + HALO - 1])[F * (HALO - 1):F * (HALO - 1 + y1 - y0)]
    codes = [rc.planes(rc.to_frame(x, "444"), "444", F * (y1 - y0), F * w)[0] for x in (whole_f, cut_f)]
    e = np.abs(cut_f.astype(np.float64) - whole_f)
    print(f"  the smooth frame, 6 halo rows: largest |difference| of the f32 output in the first / last {F} rows {219 * e[:F].max():.3f} / "
          f"{219 * e[-F:].max():.3f} of an 8-bit level; 8-bit luma samples that differ: {int((codes[0] != codes[1]).sum())} of {codes[0].size}")
