"""The C++ drop-in's RenderKernel::render_adaptive (include/render_kernel_hip.h), compiled against the
reference's own headers and objects: on Cornell its Image and tile counts equal, bit for bit, what the same
passes give through the C calls; threshold 0 gives render()'s frame; max_passes limits the adaptive passes.
Linked to the hostsim build (container only: needs /root/reference) and, built there by
`make build/adaptive_shim_test_hip`, to the product library for the GPU run, as tests/test_shim.py."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"
WANT = "ADAPTIVE_SHIM frame 1 counts 1 mixed 1 all 1 max_passes 1 throws 1"
ARGS = ["40", "30", "4"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_adaptive(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/adaptive_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([os.path.join(gio.REPO, "build", "adaptive_shim_test"), scenes.scene_path("cornell"), str(sky), *ARGS],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout


SHIM_HIP = os.path.join(gio.REPO, "build", "adaptive_shim_test_hip")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SHIM_HIP), reason="build/adaptive_shim_test_hip not built (container)")
def test_cpp_shim_adaptive_on_gfx950(tmp_path):
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([SHIM_HIP, scenes.scene_path("cornell"), str(sky), *ARGS], capture_output=True, text=True,
                       timeout=110)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout
