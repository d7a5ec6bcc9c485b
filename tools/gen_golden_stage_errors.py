"""Records tests/golden/stage_errors.json: what a hostsim build of the library answers to the calls of
tests/stage_error_cases.py, the seven frame stages' argument errors in both forms, as
{"build": rt_build_id, "cases": {"stage/form/case": [return code, rt_last_error text]}}. Run once with the
library of the commit before the stages' argument checks were gathered into csrc/rt_stage_args.h
(RT_HOSTSIM_LIB=<that build's librt_hostsim.so>); tests/test_stage_errors.py holds later builds to it.

  RT_HOSTSIM_LIB=... python tools/gen_golden_stage_errors.py [OUT]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import stage_error_cases as sec  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else sec.GOLDEN
    c = sec.Calls()
    build = c.build_id()
    c.close()
    cases = sec.run_all()
    assert list(cases) == sec.case_keys()
    with open(out, "w") as f:
        json.dump({"build": build, "cases": cases}, f, indent=0, sort_keys=False)
        f.write("\n")
    for stage in sec.STAGES:
        mine = {k: v for k, v in cases.items() if k.startswith(stage + "/")}
        print(stage, len(mine), "calls,", sum(1 for v in mine.values() if v[0] == 0), "of them RT_OK")
    print("build", build, "wrote", out, os.path.getsize(out), "bytes")
