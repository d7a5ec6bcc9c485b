"""The C++ drop-in's RenderKernel::motion_vectors and RenderKernel::motion_blur (include/render_kernel_hip.h) compiled
against the reference's own headers and objects: tests/native/motion_shim_test.cpp, a row in the pattern of
tests/test_shims.py, linked to the hostsim build of the C ABI (container only) and to the product library on the GPU."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
from test_shims import REF, STAGE, Row, _run

ROW = Row("motion_shim_test", "cornell12", "S", STAGE,
          "MOTION_SHIM vectors 1 still_camera 1 defaults 1 params 1 no_reach 1 something_moved 1 bad_max_radius_throws 1 "
          "bad_shutter_throws 1 bad_size_throws 1")


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_motion_shim_on_hostsim(manifest, tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/" + ROW.program], check=True)
    _run(ROW, os.path.join(gio.REPO, "build", ROW.program), tmp_path, manifest)


@pytest.mark.gpu
def test_motion_shim_on_gfx950(manifest, tmp_path):
    exe = os.path.join(gio.REPO, "build", ROW.program + "_hip")
    if not os.path.exists(exe):
        pytest.skip(f"build/{ROW.program}_hip not built (make shims-hip, container)")
    _run(ROW, exe, tmp_path, manifest, timeout=110)
