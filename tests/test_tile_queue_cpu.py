"""The tile-queue case table (tests/tile_queue_cases.py) without a GPU: every case is planned by the HIP-free planners (tests/c/plan_check.cpp,
built as tests/test_plan_cpu.py builds it) for the compute units the case sets, and what the case claims to reach must show in the
planner's lines -- so tests/test_gpu_tile_queue.py cannot quietly stop reaching the queue when a planner threshold moves.  Then the
queue's index arithmetic, restated in numpy: whatever the order of pulls and steals, a launch hands out every tile exactly once."""
import itertools

import numpy as np
import pytest

import plan_cases
import tile_queue_cases as tq


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    return tq.plan_table(plan_cases.build_plan_check(tmp_path_factory.mktemp("plan_check")))


def _plain(ctx):
    return [l for l in ctx if not l.startswith("#")]


def test_every_case_reaches_what_it_claims(planned):
    wrong = []
    for c in tq.TABLE:
        assert c["reach"] and set(c["reach"]) <= set(tq.PROPERTIES), c["name"]
        got = tq.reached(c, planned[c["id"]])
        if not set(c["reach"]) <= got:
            wrong.append((c["name"], sorted(set(c["reach"]) - got), _plain(planned[c["id"]])))
        assert not ("control" in c["reach"] and "queue" in got), c["name"]
    assert not wrong, wrong


def test_every_property_is_claimed_in_each_precision():
    for prec in tq.PRECISIONS:
        claimed = set().union(*(c["reach"] for c in tq.TABLE if c["precision"] == prec))
        assert claimed == set(tq.PROPERTIES), (prec, sorted(set(tq.PROPERTIES) - claimed))
    # the exact mode forks by the automatic rule (the split-half mode never does: sr_plan_fork)
    assert any("fork" in c["reach"] and "fork" not in c["set"] for c in tq.TABLE if c["precision"] == "f32")


def test_the_table_holds_what_it_was_asked_to_hold(planned):
    cases = tq.TABLE
    have = lambda **kv: [c for c in cases if all(c[k] == v for k, v in kv.items())]  # noqa: E731
    for prec in tq.PRECISIONS:
        for factor in (2, 3, 4):
            assert have(precision=prec, factor=factor)
        assert {c["io"] for c in have(precision=prec)} == {"f32", "u8"} and have(precision=prec, ch=4)
        assert have(precision=prec, n=2) and have(precision=prec, n=3)
        assert all(c["cus"] <= 2 for c in cases if c["n"] > 1)
        assert {tuple(c["halo"]) for c in have(precision=prec, call="band")} == {(7, 7), (7, 0), (0, 7)}
        assert all(c["h"] - sum(c["halo"]) >= 40 for c in have(precision=prec, call="band"))
        sets = [c["set"] for c in have(precision=prec)]
        for key, values in (("th", ("8", "4", tq.FIVE)), ("tail", ("0", "1", "2")), ("bw", ("0", "1", "2")), ("fork", ("0", "1", "14"))):
            assert {s[key] for s in sets if key in s} >= set(values), (prec, key)
        assert all(s.get("pipe") == "all" for s in sets if "th" in s)
        assert all(3 <= (c["w"] + 31) // 32 <= 5 for c in have(precision=prec) if "bw" in c["set"])
        assert {c["host"] for c in have(precision=prec, call="host")} >= {"inorder", "alternating"}
        assert all(c["cus"] <= 2 for c in have(call="host"))
    assert {c["set"]["wino"] for c in have(precision="f32") if "wino" in c["set"]} == {"0", "2"}
    # the split-half mode's last stage at factor 4 exists with 4-row tiles only
    for c in have(precision="split_f16", factor=4):
        assert all(ty8 == 0 for st, _, ty8, *_ in tq.launches_of(planned[c["id"]]) if st == 4), c["name"]
    # a host call's plan is the kind the case states
    for c in have(call="host"):
        head = _plain(planned[c["id"]])[0].split()
        assert head[0] == "host" and head[1] == (c["host"] or "one"), (c["name"], head)
    # the mildest case, the one to run alone first: 5 CUs, 61 x 97, exact f32, undivided, every XCD's queue owned
    mild = have(cus=5, precision="f32", factor=3, h=61, w=97, io="f32", set={})[0]
    assert _plain(planned[mild["id"]])[:3] == ["fork 0", "launch 0 first 8 0 32", "launch 1 pipe 6 4 10"]
    assert all(c["oracle"] == (c["h"] * c["w"] <= 61 * 97) for c in cases) and any(not c["oracle"] for c in cases)
    assert len({c["name"] for c in cases}) == len(cases)


# ---- the queue's arithmetic ----
def _launch_shapes(planned):
    shapes = set()
    for c in tq.TABLE:
        shapes |= set(tq.queue_launches(c, planned[c["id"]]))
    return shapes


def test_runs_partition_each_class():
    for ntiles in range(0, 200):
        runs = [tq.run_of_xcd(x, ntiles) for x in range(8)]
        assert runs[0][0] == 0 and sum(n for _, n in runs) == ntiles
        assert all(runs[x][0] + runs[x][1] == runs[x + 1][0] for x in range(7))
        assert max(n for _, n in runs) - min(n for _, n in runs) <= 1


def test_the_head_preset_counts_the_first_tiles():
    for grid in range(1, 600):
        heads = tq.head_preset(grid)
        assert heads == [sum(1 for b in range(grid) if b & 7 == x) for x in range(8)]


def _assert_exactly_once(nbig, nsmall, grid, rng):
    handed = tq.drain(nbig, nsmall, grid, rng)
    assert sorted(handed) == list(range(nbig + nsmall)), (nbig, nsmall, grid, handed)


def test_every_tile_is_handed_out_exactly_once_small_launches():
    """all nbig, nsmall <= 24 and grid <= 16 with grid <= tiles (sr_tile_plan: grid = min(tiles, resident)), round robin and three random orders"""
    rngs = [None] + [np.random.default_rng(s) for s in (1, 2, 3)]
    for nbig, nsmall, grid in itertools.product(range(25), range(25), range(1, 17)):
        if grid > nbig + nsmall:
            continue
        for rng in rngs:
            _assert_exactly_once(nbig, nsmall, grid, rng)


def test_every_tile_is_handed_out_exactly_once_in_the_tables_launches(planned):
    shapes = _launch_shapes(planned)
    assert any(grid < 8 and tq.nonempty_runs(nb, ns) > grid for nb, ns, grid in shapes) and any(nb and ns for nb, ns, _ in shapes)
    for nbig, nsmall, grid in sorted(shapes):
        for rng in [None] + [np.random.default_rng(10 + s) for s in range(8)]:
            _assert_exactly_once(nbig, nsmall, grid, rng)


def test_an_ownerless_queue_is_emptied_by_steals_alone():
    """grid 2 on 8 + 8 tiles: the queues of XCD 2-7 have no owner, their heads start at 0 and every one of their tiles is a steal"""
    assert tq.head_preset(2) == [1, 1, 0, 0, 0, 0, 0, 0]
    handed = tq.drain(8, 8, 2)
    owned = {tq.queue_slot(x, 8, 8, k) for x in (0, 1) for k in range(2)}
    assert owned == {0, 1, 8, 9} and sorted(handed) == list(range(16)) and len(set(handed) - owned) == 12


def test_tile_coords_is_a_bijection_under_every_block_width():
    for tiles_x, tiles_y, n, bw in itertools.product(range(1, 8), range(1, 6), (1, 2, 3), (0, 1, 2, 3, 16)):
        seen = {tq.tile_coords(t, tiles_x, tiles_y, bw) for t in range(n * tiles_x * tiles_y)}
        assert seen == set(itertools.product(range(n), range(tiles_x), range(tiles_y))), (tiles_x, tiles_y, n, bw)
    assert [tq.tile_coords(t, 5, 2, 2) for t in range(10)] == [(0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (0, 2, 0), (0, 3, 0), (0, 2, 1), (0, 3, 1),
                                                               (0, 4, 0), (0, 4, 1)]
