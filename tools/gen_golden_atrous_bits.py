"""Records tests/golden/atrous_bits.json: the SHA-256 of every output of the hostsim rt_denoise and
rt_denoise_var over the cases of tests/atrous_bits_cases.py, as {"build": rt_build_id, "cases": {"WxH/passesN/
guides|colour": {output: digest}}}. Run once with the library of the commit before the two filters were made one
(RT_HOSTSIM_LIB=<that build's librt_hostsim.so>); tests/test_atrous_bits.py holds later builds to it.

  RT_HOSTSIM_LIB=... python tools/gen_golden_atrous_bits.py [OUT]
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import atrous_bits_cases as ab  # noqa: E402
import rt_amd  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else ab.GOLDEN
    build = rt_amd.lib(True).rt_build_id().decode()
    cases = ab.run_all()
    with open(out, "w") as f:
        json.dump({"build": build, "cases": cases}, f, indent=0, sort_keys=False)
        f.write("\n")
    print("build", build, len(cases), "cases,", sum(len(v) for v in cases.values()), "digests, wrote", out,
          os.path.getsize(out), "bytes")
