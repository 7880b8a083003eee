"""The tile, fork and host-chunk planners (rusty_sr_amd/csrc/sr_plan.cpp) without a GPU.  tests/c/plan_check.cpp -- g++ alone, sr_plan.cpp
alone, ASan + UBSan -- plans every case of tests/golden/plan_cases.json for the compute units the parent's records were taken on; what
it prints must equal tests/golden/plan_records_parent.json.gz, the plan records of the library as it was BEFORE the planners moved out
of sr_api.cpp (recorded on an MI355X by tests/golden/make_plan_records.py), for every case.  Then the plans' own invariants."""
import pytest

import plan_cases

SR_HALO = plan_cases.SR_HALO


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """plan_check's exit status, stderr and output over the whole table, at the recorded CU count"""
    exe = plan_cases.build_plan_check(tmp_path_factory.mktemp("plan_check"))
    cases = plan_cases.load_cases()
    return cases, plan_cases.load_parent(), plan_cases.run_plan_check(exe, cases, plan_cases.load_parent()["cus"])


def _lines(ctx_lines):
    return [l for l in ctx_lines if not l.startswith("#")]


def test_the_planners_build_and_run_without_hip_under_sanitizers(planned):
    cases, _, (status, err, out) = planned
    assert status == 0, err
    assert sorted(out) == [c["id"] for c in cases]


def test_every_case_plans_what_the_parent_planned(planned):
    cases, parent, (status, err, out) = planned
    assert status == 0, err
    assert sorted(parent["records"]) == sorted(c["key"] for c in cases)  # none skipped, none missing
    wrong = []
    for c in cases:
        want = [plan_cases.canonical(text) for text in parent["records"][c["key"]]]
        got = [_lines(ctx) for ctx in out[c["id"]]]
        assert any(want), c  # (a record that holds nothing would pin nothing)
        if got != want:
            wrong.append((c, got, want))
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; the first: {wrong[0]}"


def test_the_table_reaches_the_rules_it_is_there_for(planned):
    """(guards the table, not the planners: the corners the shapes were chosen for do show in the parent's records)"""
    cases, parent, _ = planned
    assert parent["cus"] == 256

    def rec(call, io, h, w):  # the plain exact-f32 call of that shape, factor 3
        plain = dict(call=call, factor=3, precision="f32", io=io, n=1, h=h, w=w, halo=[0, 0], set={}, pipeline=True, profiling=False, engines=1)
        found = [c for c in cases if {k: c[k] for k in plain} == plain]
        assert len(found) == 1, (call, io, h, w)
        return plan_cases.canonical(parent["records"][found[0]["key"]][0])
    dev = lambda h, w: rec("dev", "f32", h, w)  # noqa: E731
    host = lambda h, w, io: rec("host", io, h, w)  # noqa: E731
    st = lambda lines: {int(l.split()[1]): " ".join(l.split()[3:5]) for l in lines if l.startswith("launch")}  # noqa: E731
    # 384x1024 is 3.0 rounds: the tail of 4-row tiles in stages 1 / 3, none in the Winograd stage 2 and the last stage
    assert st(dev(384, 1024)) == {0: "48 0", 1: "40 16", 2: "48 0", 3: "40 16", 4: "48 0"}
    assert st(dev(388, 1024))[2] == st(dev(388, 1024))[4] == "48 1"  # rows % 8 in 1..4: ONE row of 4-row tiles
    assert st(dev(389, 1024))[2] == st(dev(389, 1024))[4] == "49 0"
    assert dev(600, 800)[0] == "fork 1 298,302" and dev(1080, 1920)[0] == "fork 1 538,542"
    assert host(1080, 1920, "u8")[0] == "host alternating 400,400,200,80"
    assert host(1080, 1920, "f32")[0] == "host inorder 216,216,216,216,216"


def test_every_plan_covers_its_rows_and_fits_the_chip(planned):
    cases, parent, (status, err, out) = planned
    assert status == 0, err
    cus = parent["cus"]
    for c in cases:
        halo = c["halo"]
        for ctx in out[c["id"]]:
            if not ctx:
                continue
            lines = _lines(ctx)
            head = lines[0].split()
            passes = [[int(v) for v in l.split()[2:]] for l in ctx if l.startswith("# pass")]
            own = [p[0] for p in passes]
            assert all(p[1] in (0, SR_HALO) and p[2] in (0, SR_HALO) for p in passes), (c, passes)  # every halo is none or SR_HALO
            if head[0] == "host":
                sizes = [int(v) for v in head[2].split(",")]
                lo, hi = (int(v) for v in head[3][5:].split(":")) if len(head) > 3 else (0, c["h"])
                if head[1] in ("inorder", "alternating"):
                    assert sizes == own and sum(sizes) == hi - lo, (c, lines[0])   # the bands are the rows asked for
                elif head[1] == "batch":
                    assert sum(sizes) == c["n"] and all(o == c["h"] for o in own), (c, lines[0])
                else:
                    assert own == [hi - lo], (c, lines[0], own)
            else:
                want = c["h"] - halo[0] - halo[1]
                assert sum(own) == want and len(own) == (2 if head[1] == "1" else 1), (c, lines[0], own)
                if head[1] == "1":
                    assert [int(v) for v in head[2].split(",")] == own
            rows = [[int(v) for v in l.split()[2:]] for l in ctx if l.startswith("# rows")]
            launches = [l.split() for l in lines if l.startswith("launch")]
            assert len(rows) == len(launches) == 5 * len(passes)
            for (y0, y1), (_, st, form, ty8, ty4, grid) in zip(rows, launches):
                assert 8 * int(ty8) + 4 * int(ty4) >= y1 - y0 > 0, (c, st, y0, y1, ty8, ty4)  # the tiles cover the stage's rows
                assert int(grid) > 0 and (form != "pipe" or int(grid) <= 2 * cus), (c, st, form, grid)  # a persistent launch fits the chip
