"""Records tests/golden/trip_code_parent.npz: what a build of the gfx950 library does with the meshes and
rays of tests/trip_cases.py. Per mesh: the queries each probe walk leaves to the exact walk
(rt_device_queries modes 4 / 5 quads, 8 / 9 rows) and the quad walks' visit counts
(rt_device_query_trips). Run once on a GPU with the library of the commit before the branch-free push /
pop (RT_HIP_LIB=<that build with the rt_device_query_trips probe added>); the tests hold later builds to it.

  RT_HIP_LIB=... python tools/gen_golden_trip.py [OUT]
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "sycl-ray-tracing_amd"), os.path.join(REPO, "tools"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

import trip_cases as tc  # noqa: E402
from rt_amd import _capi  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else tc.GOLDEN
    d = {"build": np.array(_capi.lib().rt_build_id().decode() if hasattr(_capi.lib(), "rt_build_id") else "?")}
    for name in tc.MESHES:
        r = tc.rays(name)
        rk = tc.kernel(name, hostsim=False)
        d[f"{name}_digest"] = np.array(tc.rays_digest(name))
        for mode in (4, 5, 8, 9):
            t, _ = tc.device_queries(rk, mode, r)
            d[f"{name}_handover_{mode}"] = t == -2.0
        for any_ in (0, 1):
            d[f"{name}_trips_{any_}"] = tc.device_trips(rk, any_, r)
        cpu = tc.cpu_handovers(name)
        print(name, r.shape[0], "rays; hand-overs", {m: int(d[f"{name}_handover_{m}"].sum()) for m in (4, 5, 8, 9)},
              "cpu twin equal to quads:", bool(np.array_equal(cpu, d[f"{name}_handover_4"])),
              "calls closest / any", int(d[f"{name}_trips_0"][:, 0].sum()), int(d[f"{name}_trips_1"][:, 0].sum()))
    np.savez_compressed(out, **d)
    print("wrote", out, os.path.getsize(out), "bytes")
