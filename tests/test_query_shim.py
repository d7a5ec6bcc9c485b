"""The C++ drop-in's RenderKernel::query_closest / query_any (include/render_kernel_hip.h),
compiled against the reference's own headers and objects: on the Cornell camera rays they
give what rt_intersect gives, field for field. Linked to the hostsim build of the C ABI
(container only: needs the reference's headers, skipped elsewhere as tests/test_shim.py) and,
built in the container by `make build/query_shim_test_hip`, to the product library on the GPU."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"
SHIM_HIP = os.path.join(gio.REPO, "build", "query_shim_test_hip")


def _run(binary, timeout=None):
    r = subprocess.run([binary, scenes.scene_path("cornell"), "48", "32"], capture_output=True, text=True,
                       timeout=timeout)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "QUERY_SHIM closest 1 any 1 hits 1" in r.stdout


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_queries_equal_rt_intersect():
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/query_shim_test"], check=True)
    _run(os.path.join(gio.REPO, "build", "query_shim_test"))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SHIM_HIP), reason="build/query_shim_test_hip not built (make build/query_shim_test_hip, container)")
def test_cpp_shim_queries_on_gfx950_equal_rt_intersect():
    _run(SHIM_HIP, timeout=110)
