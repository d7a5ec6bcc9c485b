"""The C++ drop-in's RenderKernel::meter and RenderKernel::auto_exposure (include/render_kernel_hip.h) against the C
calls, on the hostsim build (container only: it needs /root/reference, skipped elsewhere as
tests/test_firefly_shim.py). make sanitize-meter builds the same stand-alone program with ASan and UBSan over the
hostsim sources and runs it."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_meter_and_auto_exposure_equal_c_abi(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/meter_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    exe = os.path.join(gio.REPO, "build", "meter_shim_test")
    for sky_arg in (str(sky), "-"):
        r = subprocess.run([exe, scenes.scene_path("cornell12"), sky_arg, "33", "21", "3"], capture_output=True, text=True)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "METER_SHIM hist 1 counts 1 defaults 1 params 1 empty 1 bad_params_throw 1" in r.stdout
