"""The C++ drop-in's RenderKernel::progress_track_noise, progress_noise and render_progressive_tracked
(include/render_kernel_hip.h), compiled against the reference's own headers and objects: on Cornell the
struct a callback reads equals a second kernel's for the same passes, a query after one pass throws, the
tracked frame is render()'s Image bit for bit and a threshold stops the passes. Linked to the hostsim build
(container only: needs /root/reference) and, built there by `make build/noise_test_hip`, to the product
library for the GPU run, as tests/test_shim.py."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"
WANT = "NOISE_SHIM frame 1 one_pass_throws 1 agree 1 sane 1 stops 1 untracked_throws 1"
ARGS = ["40", "30", "4"]


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_noise(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/noise_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([os.path.join(gio.REPO, "build", "noise_test"), scenes.scene_path("cornell"), str(sky), *ARGS],
                       capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout


SHIM_HIP = os.path.join(gio.REPO, "build", "noise_test_hip")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SHIM_HIP), reason="build/noise_test_hip not built (container)")
def test_cpp_shim_noise_on_gfx950(tmp_path):
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([SHIM_HIP, scenes.scene_path("cornell"), str(sky), *ARGS], capture_output=True, text=True,
                       timeout=110)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout
