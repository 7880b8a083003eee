"""The built library plans what the HIP-free planners plan: every case of tests/golden/plan_cases.json is run once on the GPU and its plan
record (sr_get_experiment "plan") compared with what tests/c/plan_check.cpp prints for this device's compute units.  On a 256-CU device
that is the parent's record (tests/test_plan_cpu.py); on any other partition it still holds sr_api.cpp to sr_plan.cpp.  The words of
each launch line that describe the call -- prec, f, img, out, ch -- are checked against the call's own arguments.  (plan_check is built
plain here: its run under ASan and UBSan is the CPU test's.)"""
import pytest

import plan_cases

pytestmark = pytest.mark.gpu


def test_the_library_runs_the_plans_of_the_planner_module(tmp_path):
    from rusty_sr_amd.engine import parse_plan
    cases = plan_cases.load_cases()
    run = plan_cases.Runner()
    try:
        cus = run.cus()
        records = {c["id"]: run.run(c) for c in cases}
    finally:
        run.close()
    status, err, planned = plan_cases.run_plan_check(plan_cases.build_plan_check(tmp_path, sanitize=False), cases, cus)
    assert status == 0, err
    wrong = []
    for c in cases:
        got = [plan_cases.canonical(text) for text in records[c["id"]]]
        want = [[l for l in ctx if not l.startswith("#")] for ctx in planned[c["id"]]]
        assert any(got), c
        if got != want:
            wrong.append((c, got, want))
        io = c["io"]
        for text in records[c["id"]]:
            for l in parse_plan(text)["launches"]:
                assert (l["prec"], l["f"], l["img"], l["out"], l["ch"]) == (c["precision"], c["factor"], io, io, 3), (c, l)
    assert not wrong, f"{cus} CUs: {len(wrong)} of {len(cases)} cases differ; the first: {wrong[0]}"
