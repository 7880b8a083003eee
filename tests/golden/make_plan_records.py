"""Record tests/golden/plan_records_parent.json.gz: what a build of libsrhip plans for every case of tests/golden/plan_cases.json -- the
text of sr_get_experiment("plan") after each call, verbatim, and the compute units of the device it planned for.

    SRHIP_LIB=/path/to/libsrhip.so python tests/golden/make_plan_records.py [--out FILE]     # needs the GPU
    python tests/golden/make_plan_records.py --show                                          # the committed records as text

The committed file was recorded once, on an MI355X (256 CUs), from a library built from the commit BEFORE the tile, fork and host-chunk
planners moved out of sr_api.cpp into sr_plan.cpp: it pins what that move had to reproduce (tests/test_plan_cpu.py) and is never
regenerated from the code it checks.  Each call is made once, on all-zero pixels, with the fork tuner off ("forktune" = "0")."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import plan_cases  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=plan_cases.PARENT)
    ap.add_argument("--show", action="store_true", help="print the committed records (the file is gzipped: 380 KB of text) and stop")
    a = ap.parse_args()
    if a.show:
        blob = plan_cases.load_parent()
        print("cus", blob["cus"])
        for key, texts in blob["records"].items():
            print("\n".join([key] + [f"  ctx {k}: {line}" for k, text in enumerate(texts) for line in text.splitlines()]))
        return
    run = plan_cases.Runner()
    records = {c["key"]: run.run(c) for c in plan_cases.load_cases()}
    blob = {"cus": run.cus(), "records": records}
    run.close()
    plan_cases.save_records(a.out, blob)
    print(f"{len(records)} cases, {blob['cus']} CUs -> {a.out}")


if __name__ == "__main__":
    main()
