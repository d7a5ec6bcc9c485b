"""The C++ drop-in's RenderKernel::temporal_accumulate (include/render_kernel_hip.h), compiled against the
reference's own headers and objects and linked to the hostsim build of the C ABI: its outputs over two
frames under a moved camera equal rt_render_features + rt_temporal_accumulate called directly, bit for
bit. Container only: needs /root/reference (skipped elsewhere, as tests/test_denoise_shim.py)."""
from __future__ import annotations

import os
import subprocess

import pytest

import golden_io as gio
import scenes

REF = "/root/reference/include"


@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_temporal_accumulate_equals_c_abi(tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/temporal_shim_test"], check=True)
    sky = tmp_path / "sky.raw"
    scenes.write_sky_raw(str(sky), "S")
    r = subprocess.run([os.path.join(gio.REPO, "build", "temporal_shim_test"), scenes.scene_path("cornell12"), str(sky),
                        "33", "21", "3"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "TEMPORAL_SHIM first 1 second 1 accumulated 1 bad_size_throws 1" in r.stdout
