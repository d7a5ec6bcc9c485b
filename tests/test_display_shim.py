"""The C++ drop-in's RenderKernel::render_linear, display and write_image_hdr
(include/render_kernel_hip.h), compiled against the reference's own headers and objects: on Cornell,
display(render_linear()) equals render()'s Image bit for bit, and the .hdr file it writes reads back
through rt_read_hdr. Linked to the hostsim build (container only: needs /root/reference) and, built
there by `make build/display_shim_test_hip`, to the product library for the GPU run, as
tests/test_shim.py."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"
WANT = "DISPLAY_SHIM round_trip 1 alpha 1 linear_differs 1 exposure 1 explicit 1 hdr 1"
ARGS = ["40", "30", "4"]


def _hdr_reads_back(path):
    import rt_amd
    img = rt_amd.read_image_float(str(path))
    assert (img.width, img.height) == (40, 30)
    assert np.isfinite(img.pixels).all() and img.pixels[..., :3].max() > 0


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_display(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/display_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    out = tmp_path / "linear.hdr"
    r = subprocess.run([os.path.join(gio.REPO, "build", "display_shim_test"), scenes.scene_path("cornell"), str(sky),
                        *ARGS, str(out)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout
    _hdr_reads_back(out)


SHIM_HIP = os.path.join(gio.REPO, "build", "display_shim_test_hip")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SHIM_HIP), reason="build/display_shim_test_hip not built (container)")
def test_cpp_shim_display_on_gfx950(tmp_path):
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    out = tmp_path / "linear.hdr"
    r = subprocess.run([SHIM_HIP, scenes.scene_path("cornell"), str(sky), *ARGS, str(out)], capture_output=True, text=True,
                       timeout=110)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert WANT in r.stdout
    _hdr_reads_back(out)
