"""The noise estimate of a tracked progression on the hostsim build: the cases of tests/noise_cases.py and the
command line. The GPU half (tests/test_noise_gpu.py) holds k_noise_fold and k_noise_tiles to the same numpy
restatement and to this build, bit for bit."""
from __future__ import annotations

import os
import re
import subprocess
import sys

import pytest

import noise_cases as nc

import rt_amd


@pytest.mark.parametrize("which", ["ordinary", "edge"])
@pytest.mark.parametrize("halves", nc.HALVES, ids=lambda h: f"{h[0]}+{h[1]}")
@pytest.mark.parametrize("shape", nc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_model_by_injected_state(shape, halves, which):
    nc.case_model(True, shape, halves, which)


@pytest.mark.parametrize("split", nc.SPLITS, ids=str)
@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_fold(scene, split):
    nc.case_fold(True, scene, split)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("split", nc.SPLITS, ids=str)
def test_tracking_changes_no_frame(split, device):
    nc.case_same_frame(True, split, device)


def test_checkpoint():
    nc.case_checkpoint(True)


def test_row_shard():
    nc.case_shard(True)


def test_errors_and_state():
    nc.case_errors(True)


def test_it_measures_noise():
    nc.case_measures_noise(True)


def test_python_render_kernel():
    nc.case_python(True)


# ------------------------------------------------------------------ the command line
def test_cli_noise_threshold(tmp_path):
    """--noise-threshold=0 runs every pass and writes the four PNGs of a run without the flag, byte for byte;
    a threshold above the first reported max_tile stops after the second pass; the flag needs --preview-every."""
    import scenes

    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    names = ["RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png"]
    w, h, spp, nb = 16, 12, 4, 2

    def run(out, *flags, code=0):
        r = subprocess.run([sys.executable, "-m", "rt_amd.cli", scenes.scene_path("cornell12"), f"--sky={hdr}", f"--w={w}",
                            f"--h={h}", f"--samples={spp}", f"--bounces={nb}", "--hostsim", "--camera=cornell",
                            f"--out={out}", *flags], capture_output=True, text=True, env=env)
        assert r.returncode == code, r.stdout + r.stderr
        return r.stdout

    plain, prog, all_passes, early = (tmp_path / n for n in ("plain", "prog", "all", "early"))
    run(plain)
    run(prog, "--preview-every=1")
    out = run(all_passes, "--preview-every=1", "--noise-threshold=0")
    lines = re.findall(r"^noise: done (\d+) max_tile (\S+) tiles_over (\d+)$", out, flags=re.M)
    assert [int(d) for d, _, _ in lines] == [2, 3, 4], out
    assert all(int(over) > 0 for _, _, over in lines), "at threshold 0 every pass leaves tiles over it"
    for n in names:
        assert (all_passes / n).read_bytes() == (plain / n).read_bytes(), n
    for k in range(1, spp + 1):
        assert (all_passes / f"RT_preview_{k}.png").read_bytes() == (prog / f"RT_preview_{k}.png").read_bytes(), k
    first_max = float(lines[0][1])
    out = run(early, "--preview-every=1", f"--noise-threshold={first_max * 2 + 1}")
    lines = re.findall(r"^noise: done (\d+) max_tile (\S+) tiles_over (\d+)$", out, flags=re.M)
    assert lines == [("2", lines[0][1], "0")] and float(lines[0][1]) == first_max, out
    assert sorted(p.name for p in early.glob("RT_preview_*.png")) == ["RT_preview_1.png", "RT_preview_2.png"]
    assert (early / names[0]).read_bytes() == (prog / "RT_preview_2.png").read_bytes(), "the frame of the samples done so far"
    assert all((early / n).exists() for n in names)
    run(tmp_path / "bad", "--noise-threshold=0.1", code=2)
