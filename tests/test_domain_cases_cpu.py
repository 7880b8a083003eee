"""The gate of tests/domain_cases.py, on the oracle alone (no GPU): every case is what it claims to be.  In the over leg exactly one
value of exactly the intended node reaches 65504, at (P, b); in the under leg none does; every other split value is far below the
limit, so a flag can only come from that one value; and, for the nodes an expand convolution reads, a kernel that let the value
saturate at 65504 would miss the output bar of tests/test_gpu_domain_nodes.py -- the check is not the only thing that stands between
a clamped pixel and a green suite, but the table proves it would be seen."""
import numpy as np
import pytest

import domain_cases as dc
import oracle


def _split_values(c):
    return {k: np.abs(c.t64[k]) for k in dc.NODES}


@pytest.mark.parametrize("row", dc.TABLE, ids=dc.table_id)
def test_one_value_of_one_node_and_nothing_else(row):
    node, pos, b, factor = row
    for leg in dc.LEGS:
        c = dc.case(node, pos, b, leg, factor)
        mags = _split_values(c)
        y, x = c.P
        peak = float(mags[node][y, x, b])
        assert peak == mags[node].max()
        assert abs(peak - dc.LEGS[leg] * dc.LIMIT) <= 2e-4 * dc.LIMIT, (c.id, peak)
        beyond = {k: int((m >= dc.LIMIT).sum()) for k, m in mags.items()}
        assert beyond == {k: int(leg == "over" and k == node) for k in dc.NODES}, (c.id, beyond)
        # the f32 oracle sees the same peak, and a finite output
        p32 = float(np.abs(c.t32[node]).max())
        assert abs(p32 - peak) <= 1e-5 * peak, (c.id, p32, peak)
        assert np.isfinite(c.o64).all() and np.isfinite(c.o32).all()
        # nothing else comes near the limit
        others = 0.0
        for k, m in mags.items():
            m = m.copy()
            if k == node:
                m[y, x, b] = 0
            others = max(others, float(m.max()))
        print(f"{c.id}: g {c.g:.6g}  peak {peak / dc.LIMIT:.4f}  largest other split value {others / dc.LIMIT:.4f} of the limit  max|out| {np.abs(c.o64).max():.4g}")
        assert others <= dc.OTHERS_BAR * dc.LIMIT, (c.id, others)
        # the input itself is an ordinary u8 image
        assert c.x.max() == 1.0 and c.x[0, y, x, 0] == 1.0
        if node != "f":
            bar = dc.OUT_TOL * float(np.abs(c.o64).max())
            off = dc.saturated_output_error(c)
            print(f"{c.id}: saturated output off by {off:.4g}, the output bar is {bar:.4g}")
            assert off > 10 * bar, (c.id, off, bar)


@pytest.mark.parametrize("row", [r for r in dc.TABLE if r[0] != "f" and r[2] == 31], ids=dc.table_id)
def test_the_expand_restatement_is_the_oracles(row):
    """expand_of_channel against the oracle: the two legs differ in g alone, so in channel b of the node alone, and their outputs by
    what the expand convolution makes of that difference."""
    node, pos, b, factor = row
    over, under = dc.case(node, pos, b, "over", factor), dc.case(node, pos, b, "under", factor)
    dmap = over.t64[node][:, :, b] - under.t64[node][:, :, b]
    for k in dc.NODES:   # (nothing else moved)
        rest = over.t64[k] - under.t64[k]
        if k == node:
            rest = np.delete(rest, b, axis=2)
        assert np.abs(rest).max() == 0
    want = over.o64[0] - under.o64[0]
    got = dc.expand_of_channel(over, dmap)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    assert np.abs(want).max() > 1.0


def test_boundary_inputs():
    p = dc.boundary_params()
    for which, (v, leaves) in dc.BOUNDARY.items():
        x = dc.boundary_image(which)
        big = np.abs(x) >= dc.LIMIT
        assert int(big.sum()) == int(leaves)
        y, xx, ch = dc.BOUNDARY_AT
        assert x[0, y, xx, ch] == np.float32(v) and np.isfinite(x).all()
        rest = np.abs(x).copy()
        rest[0, y, xx, ch] = 0
        assert rest.max() < 0.25
        nodes = dc.nodes_f64(p, x)
        top = max(float(np.abs(m).max()) for m in nodes.values())
        print(f"boundary {which}: sample {v!r}, largest node value {top:.4g}")
        assert top < dc.OTHERS_BAR * dc.LIMIT
        assert np.isfinite(oracle.forward(p, x, f64=True)).all()
    assert dc.LIMIT - 0.01 < dc.BELOW < dc.LIMIT
    # round toward zero to a half: the float just below 65504 lands on 0x7bfe (65472), one pattern short of the limit's
    h = np.float32(dc.BELOW).astype(np.float16)
    if float(h) > dc.BELOW:
        h = np.nextafter(h, np.float16(0))
    assert h.view(np.uint16) == 0x7bfe
