"""The C++ drop-in (include/render_kernel_hip.h) compiled against the REFERENCE's own headers and objects: the
stand-alone programs of tests/native/ (shim_test.cpp and the *_shim_test.cpp files over shim_common.h), each of
which drives one part of the drop-in as the reference's main.cpp drives render_kernel.h, holds it to the C ABI or
to render() bit for bit, prints one verdict line and returns 0 when every check held. ROWS is every invocation;
each runs linked to the hostsim build of the C ABI (container only: building needs /root/reference, skipped
elsewhere) and, built there by `make shims-hip`, linked to the product library on the GPU, where the binary reads
nothing of the reference. A new check is one program, one row here and one name in the Makefile's SHIM_PROGS."""
from __future__ import annotations

import json
import os
import subprocess
from typing import Callable, NamedTuple, Optional

import numpy as np
import pytest

import golden_io as gio
import rt_cases
import scenes

REF = "/root/reference/include"
with open(os.path.join(gio.GOLDEN, "manifest.json")) as _f:
    CFG1 = json.load(_f)["renders"]["cfg1_cornell12"]


def _cfg1_frame_is_the_golden(out, manifest):
    """shim_test's frame file: the compiled reference's Cfg1 golden bit for bit."""
    e = rt_cases.golden_case("cfg1_cornell12", manifest)
    fb = np.fromfile(out, dtype="<f4").reshape(e["H"], e["W"], 4)
    np.testing.assert_array_equal(fb.view(np.uint32), e["expected"].view(np.uint32))


def _hdr_reads_back(out, manifest):
    import rt_amd
    img = rt_amd.read_image_float(str(out))
    assert (img.width, img.height) == (40, 30)
    assert np.isfinite(img.pixels).all() and img.pixels[..., :3].max() > 0


class Row(NamedTuple):
    program: str
    scene: str
    sky: Optional[str]  # a scenes.write_sky_raw kind, "-" (the program's flat grey sky) or None (no sky argument)
    args: list
    want: str  # must appear in stdout
    out: Optional[str] = None  # a file under tmp_path, passed as the last argument
    check: Optional[Callable] = None  # check(out, manifest) after the run

    @property
    def id(self):
        doubled = sum(r.program == self.program for r in ROWS) > 1
        return self.program + ("-" + {"-": "flat"}.get(self.sky, self.sky) if doubled else "")


STAGE = ["33", "21", "3"]
ROWS = [
    Row("shim_test", CFG1["scene"], CFG1["sky"], [CFG1["camera"], *(str(CFG1[k]) for k in ("W", "H", "spp", "bounces"))],
        "materials_by_reference 1 changed 1 pixel 1 threaded 1", "fb.f32", _cfg1_frame_is_the_golden),
    Row("denoise_shim_test", "cornell12", "S", ["33", "21", "2", "3"], "DENOISE_SHIM blend1 1 blend075 1 filtered 1 alpha 1"),
    Row("query_shim_test", "cornell", None, ["48", "32"], "QUERY_SHIM closest 1 any 1 hits 1"),
    Row("progress_shim_test", "cornell", "S", ["40", "30", "4"],
        "PROGRESS_SHIM calls 1 image 1 preview_differs 1 final 1 stopped 1"),
    Row("display_shim_test", "cornell", "S", ["40", "30", "4"],
        "DISPLAY_SHIM round_trip 1 alpha 1 linear_differs 1 exposure 1 explicit 1 hdr 1", "linear.hdr", _hdr_reads_back),
    Row("noise_shim_test", "cornell", "S", ["40", "30", "4"],
        "NOISE_SHIM frame 1 one_pass_throws 1 agree 1 sane 1 stops 1 untracked_throws 1"),
    Row("adaptive_shim_test", "cornell", "S", ["40", "30", "4"],
        "ADAPTIVE_SHIM frame 1 counts 1 mixed 1 all 1 max_passes 1 throws 1"),
    Row("dnv_shim_test", "cornell12", "S", STAGE,
        "DNV_SHIM one_pass_throws 1 sigma 1 resolved 1 blend1 1 blend075 1 sigma_out 1 filtered 1 bad_size_throws 1"),
    Row("temporal_shim_test", "cornell12", "S", STAGE, "TEMPORAL_SHIM first 1 second 1 accumulated 1 bad_size_throws 1"),
    Row("firefly_shim_test", "cornell12", "S", STAGE,
        "FIREFLY_SHIM defaults 1 params 1 no_sigma 1 clamped 1 bad_size_throws 1 sigma_out_without_sigma_throws 1"),
    Row("meter_shim_test", "cornell12", "S", STAGE, "METER_SHIM hist 1 counts 1 defaults 1 params 1 empty 1 bad_params_throw 1"),
    Row("meter_shim_test", "cornell12", "-", STAGE, "METER_SHIM hist 1 counts 1 defaults 1 params 1 empty 1 bad_params_throw 1"),
    Row("upscale_shim_test", "cornell12", "S", STAGE, "UPSCALE_SHIM frame 1 sigma 1 params 1 finite 1 bad_arguments_throw 4"),
    Row("upscale_shim_test", "cornell12", "-", ["40", "30", "3"],
        "UPSCALE_SHIM frame 1 sigma 1 params 1 finite 1 bad_arguments_throw 4"),
]
every_row = pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])


def _run(row, exe, tmp_path, manifest, timeout=None):
    argv = [exe, scenes.scene_path(row.scene)]
    if row.sky is not None:
        argv.append("-" if row.sky == "-" else scenes.write_sky_raw(str(tmp_path / "sky.raw"), row.sky))
    out = tmp_path / row.out if row.out else None
    argv += row.args + ([str(out)] if out else [])
    r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert row.want in r.stdout
    if row.check:
        row.check(out, manifest)


@every_row
@pytest.mark.skipif(not os.path.isdir(REF), reason="needs the reference's headers (container only)")
def test_cpp_shim_on_hostsim(row, manifest, tmp_path):
    subprocess.run(["make", "-C", gio.REPO, "-s", "ref", "build/" + row.program], check=True)
    _run(row, os.path.join(gio.REPO, "build", row.program), tmp_path, manifest)


@every_row
@pytest.mark.gpu
def test_cpp_shim_on_gfx950(row, manifest, tmp_path):
    exe = os.path.join(gio.REPO, "build", row.program + "_hip")
    if not os.path.exists(exe):
        pytest.skip(f"build/{row.program}_hip not built (make shims-hip, container)")
    _run(row, exe, tmp_path, manifest, timeout=110)
