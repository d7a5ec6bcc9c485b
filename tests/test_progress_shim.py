"""The C++ drop-in's RenderKernel::render_progressive (include/render_kernel_hip.h), compiled
against the reference's own headers and objects: Cornell in passes of 2 of 6 samples, the callback
sees 2, 4, 6, and the final Image equals render()'s bit for bit. Linked to the hostsim build
(container only: needs /root/reference) and, built there by `make build/progress_shim_test_hip`,
to the product library for the GPU run, as tests/test_shim.py."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"
WANT = "PROGRESS_SHIM calls 1 image 1 preview_differs 1 final 1 stopped 1"
ARGS = ["40", "30", "4"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_render_progressive(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/progress_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([os.path.join(gio.REPO, "build", "progress_shim_test"), scenes.scene_path("cornell"), str(sky),
                        *ARGS], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout


SHIM_HIP = os.path.join(gio.REPO, "build", "progress_shim_test_hip")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SHIM_HIP), reason="build/progress_shim_test_hip not built (container)")
def test_cpp_shim_render_progressive_on_gfx950(tmp_path):
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([SHIM_HIP, scenes.scene_path("cornell"), str(sky), *ARGS], capture_output=True, text=True,
                       timeout=110)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout
