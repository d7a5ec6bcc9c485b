"""The C++ drop-in's RenderKernel::upscale (include/render_kernel_hip.h) against the C calls, on the hostsim build
(container only: it needs /root/reference, skipped elsewhere as tests/test_meter_shim.py). make sanitize-upscale builds
the same stand-alone program with ASan and UBSan over the hostsim sources and runs it."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_upscale_equals_c_abi(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/upscale_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    exe = os.path.join(gio.REPO, "build", "upscale_shim_test")
    for sky_arg, w, h in ((str(sky), "33", "21"), ("-", "40", "30")):
        r = subprocess.run([exe, scenes.scene_path("cornell12"), sky_arg, w, h, "3"], capture_output=True, text=True)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "UPSCALE_SHIM frame 1 sigma 1 params 1 finite 1 bad_arguments_throw 4" in r.stdout
