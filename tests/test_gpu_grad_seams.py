"""The backward pass (include/srhip.h sr_pair_backprop_*, rusty_sr_amd/csrc/sr_grad.hip) held to its f64 restatement at every seam of its
split sums, by impulses of error (tests/grad_seam_cases.py; the premises: tests/test_grad_seams_cpu.py).

Every row is one call with +-A on the HR samples of one LR pixel beside a seam (case D: of all its pixels, cones disjoint).  It reads the
`grad` line the call left in the plan record, asserts from that line -- the split the library used, not the table -- that each impulse
pixel sits where the case says, then compares the gradient at the bars of test_gpu_backprop.assert_grad_close and err_sum at the 1e-6
of test_gradient_matches_restatement.  The rows run SR_LOSS_MSE only (grad_seam_cases: under L1 and Charbonnier the rounding noise of
every other pixel would weigh as much as the impulse).

The noise gate, per case: the GPU's forward pass differs from the f64 one by its f32 rounding, a faint error at every pixel; one call
without an impulse gives the gradient of that alone, and its norm must be at most 0.1 of the bar of every impulse row, segment by
segment.  test_noise_gate prints what it measured."""
import numpy as np
import pytest
import torch

import grad_ref
import grad_seam_cases as gs
from test_gpu_backprop import assert_grad_close

pytestmark = pytest.mark.gpu

NOISE = 0.1     # the impulse-free gradient against the bar
STOOD = {}      # row id -> (the tags its pixels carried by the `grad` line of its call, that line)


@pytest.fixture(scope="module")
def engines():
    import rusty_sr_amd as r
    made = {}

    def get(factor, precision="f32"):
        k = (factor, precision)
        if k not in made:
            made[k] = r.Engine(gs.synthetic_params(factor, 100 + factor), device=0, factor=factor, precision=precision)
        return made[k]
    yield get
    for e in made.values():
        e.close()


def call(eng, case, weights, linear, px):
    """sr_pair_backprop_f32 on the case's LR batch and its HR batch with impulses at px -> (err_sum, n_elems, grad, the `grad` line)"""
    c = gs.CASES[case]
    err, ne, g = eng.backprop_pair(gs.lr_batch(case), gs.hr_batch(case, weights, px), gs.weights_of(case, weights), linear_loss=linear,
                                   loss_scale=gs.LOSS_SCALE)
    lines = eng.last_plan().get("grad", [])
    assert len(lines) == 1 and lines[0]["count"] == 1, eng.get_experiment("plan")
    line = lines[0]
    assert (line["n"], line["h"], line["w"]) == (c["n"], c["H"], c["W"]), line
    assert ne == 3 * c["f"] ** 2 * c["NP"]
    return err, ne, g, line


def seg(g, f, name):
    off, n, _ = grad_ref.segments(f)[name]
    return g[off:off + n].astype(np.float64)


GATES = [("A", "synthetic", False), ("A", "imagenet", False), ("A", "synthetic", True), ("B", "synthetic", False), ("C", "synthetic", False),
         ("D", "synthetic", False)]


@pytest.mark.parametrize("case,weights,linear", GATES, ids=[f"{c}-{w}" + ("-linear" if l else "") for c, w, l in GATES])
def test_noise_gate(engines, case, weights, linear):
    f = gs.CASES[case]["f"]
    _, _, g0, _ = call(engines(f), case, weights, linear, ())
    rows = [r for r in gs.ROWS if r[:3] == (case, weights, linear)]
    assert rows
    print(f"\nnoise gate, case {case} ({weights}{', linear_loss' if linear else ''}), A = {gs.AMPLITUDE:g}, {len(rows)} rows: "
          f"segment | impulse-free norm | smallest impulse norm | largest ratio to the bar (allowed {NOISE})")
    worst = []
    for name in grad_ref.segments(f):
        n0 = np.linalg.norm(seg(g0, f, name))
        wants = [seg(gs.reference(case, weights, linear, gs.pixels(r))[1], f, name) for r in rows]
        ratios = [n0 / gs.norm_bar(w) for w in wants]
        k = int(np.argmax(ratios))
        print(f"  {name:12s} {n0:.3e}  {min(np.linalg.norm(w) for w in wants):.3e}  {ratios[k]:.4f}  ({gs.row_id(rows[k])})")
        worst.append((ratios[k], name, gs.row_id(rows[k])))
    assert max(worst)[0] <= NOISE, max(worst)


@pytest.mark.parametrize("row", gs.ROWS, ids=gs.row_id)
def test_impulse_at_a_seam(engines, row):
    case, weights, linear, px = row
    f = gs.CASES[case]["f"]
    err, _, g, line = call(engines(f), case, weights, linear, gs.pixels(row))
    stood = set()
    for p, tags in px:   # where the pixel sits by the split the library used
        have = gs.stands_on(p, line)
        assert tags <= have, ("the impulse is no longer at its seam", p, sorted(tags - have), line)
        stood |= have
    STOOD[gs.row_id(row)] = (stood, line)
    want_err, want = gs.reference(case, weights, linear, gs.pixels(row))
    assert np.isfinite(g).all()
    assert_grad_close(g, want, f, gs.row_id(row))
    assert abs(err - want_err) <= 1e-6 * want_err, (err, want_err)


@pytest.mark.parametrize("p", [294, 295])
def test_entry_points_give_the_same_bits(engines, p):
    """case A beside its weight-chunk seam: the host call twice, a split_f16 context (backprop does not consult the precision), and --
    there is no f32 device form of the pair call -- sr_pair_backprop_rgba8_dev against sr_pair_backprop_rgba8 on a u8 batch of case A's
    shape with the same impulse pixel, both held to the restatement as well"""
    c = gs.CASES["A"]
    f, w = c["f"], gs.weights_of("A")
    eng = engines(f)
    a = call(eng, "A", "synthetic", False, (p,))
    b = call(eng, "A", "synthetic", False, (p,))
    s = call(engines(f, "split_f16"), "A", "synthetic", False, (p,))
    for other in (b, s):
        assert other[0] == a[0] and np.array_equal(other[2], a[2]) and other[3] == a[3]
    assert_grad_close(a[2], gs.reference("A", "synthetic", False, (p,))[1], f, ("f32", p))
    # u8: the LR batch and the impulse-free HR batch as bytes, the impulse pixel's samples at 0 or 255
    lr8 = np.round(gs.lr_batch("A") * 255).astype(np.uint8)
    hr8 = np.round(np.clip(gs.base_hr("A"), 0, 1) * 255).astype(np.uint8)
    y, x = divmod(p, c["W"])
    own = hr8[0, f * y:f * y + f, f * x:f * x + f, :]
    own[...] = np.where(own < 128, 255, 0)
    host = eng.backprop_pair(lr8, hr8, w, loss_scale=gs.LOSS_SCALE)
    line = eng.last_plan()["grad"]
    err_d, g_d = eng.backprop_pair_dev(torch.from_numpy(lr8).cuda(), torch.from_numpy(hr8).cuda(), torch.from_numpy(w).cuda(),
                                       loss_scale=gs.LOSS_SCALE)
    assert eng.last_plan()["grad"] == line == [a[3]]
    torch.cuda.synchronize()
    assert err_d.item() == host[0] and np.array_equal(g_d.cpu().numpy(), host[2])
    x8 = (lr8.astype(np.float32) / np.float32(255)).astype(np.float64)
    want_err, _, want = grad_ref.backprop(w, hr8, f, False, gs.LOSS_SCALE, 0.0, x=x8)
    assert_grad_close(host[2], want, f, ("u8", p))
    assert abs(host[0] - want_err) <= 1e-6 * want_err
    STOOD[f"A-{p}-u8-dev"] = (gs.stands_on(p, line[0]), line[0])


REACHED = {   # what the rows of each case must have stood on, by the lines of their own calls
    "A": {"wgrad:chunk:last", "wgrad:chunk:first", "wgrad:chunk:unpaired", "wgrad:chunk:midrow", "conv:workgroup:last", "conv:workgroup:first",
          "loss:partial:last", "loss:partial:first", "tail"},
    "B": {"image:seam:last", "image:seam:first", "image:lastrow", "image:firstrow", "conv:wave:last", "conv:wave:first", "wgrad:chunk:last",
          "wgrad:chunk:first", "wgrad:chunk:unpaired"},
    "C": {"colsum:chunk:last", "colsum:chunk:first", "wgrad:chunk:last", "wgrad:chunk:first"},
    "D": {"wgrad:capped", "wgrad:chunk:last", "wgrad:chunk:first", "wgrad:chunk:unpaired", "colsum:chunk:last", "colsum:chunk:first", "tail"},
}


def test_coverage_table():
    """Prints which seam of which kernel each row stood on (kernel:seam:side, grad_seam_cases.stands_on) and the split its call used,
    and holds the rows that ran to the seams their case is for."""
    lines = ["| row | wchunks x wchunk | cchunks x cchunk | conv | loss | stood on |"]
    for rid, (tags, g) in STOOD.items():
        lines.append(f"| {rid} | {g['wchunks']} x {g['wchunk']} | {g['cchunks']} x {g['cchunk']} | {g['conv']} | {g['loss']} | "
                     + " ".join(sorted(tags)) + " |")
    print("\n" + "\n".join(lines))
    ran = {gs.row_id(r) for r in gs.ROWS} & set(STOOD)
    for case, need in REACHED.items():
        ids = {gs.row_id(r) for r in gs.ROWS if r[0] == case}
        if ids <= ran:   # (a run of single rows holds nothing here)
            have = set().union(*(STOOD[i][0] for i in ids))
            assert need <= have, (case, sorted(need - have))
