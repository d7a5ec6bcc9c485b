"""Progressive rendering on the hostsim build: the cases of tests/progress_cases.py. The state
machine's pause and resume, the resolve, the checkpoint and the C ABI's checks are the code both
builds compile; the GPU half (tests/test_progress_gpu.py) adds the wave plans."""
from __future__ import annotations

import pytest

import progress_cases as pc


@pytest.mark.parametrize("split", pc.SPLITS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("scene", pc.SCENES)
def test_split_invariance(scene, split):
    pc.case_split(True, scene, split, base="random" if split == [3, 1, 2] else "blank")


def test_row_shard():
    pc.case_shard(True)


@pytest.mark.parametrize("scene", ["cornell", "fan"])
def test_seed31_line(scene):
    pc.case_seed31(True, scene)


@pytest.mark.parametrize("schedule", ["spec_cam0", "spec_cam1", "spec_cam2"])
def test_schedules(schedule):
    pc.case_schedule(True, schedule)


def test_schedule_change_between_passes():
    pc.case_schedule_change(True)


def test_edges():
    pc.case_edges(True)


def test_resolve_is_pure():
    pc.case_pure(True)


def test_interleaving():
    pc.case_interleave(True)


def test_checkpoint():
    pc.case_checkpoint(True)


def test_invalidation():
    pc.case_invalidation(True)


def test_errors():
    pc.case_errors(True)


def test_python_render_kernel():
    pc.case_python(True)


def test_cli_previews_and_checkpoint(tmp_path):
    """--preview-every=2 of 6 samples writes three previews and the same four PNGs as a run without
    the flag, byte for byte; --checkpoint resumes a finished file without rendering and ends alike."""
    import os
    import subprocess
    import sys

    import rt_amd
    import scenes

    hdr = tmp_path / "sky.hdr"
    with open(hdr, "wb") as f:  # a tiny flat Radiance file: 4 x 2 texels of (0.5, 0.5, 0.5)
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 4\n" + bytes([128, 128, 128, 128]) * 8)
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(rt_amd.__file__)))
    names = ["RT_output.png", "RT_output_denoised_1.png", "RT_output_denoised_0.75.png", "RT_output_denoised_0.5.png"]

    def run(out, *flags):
        r = subprocess.run([sys.executable, "-m", "rt_amd.cli", scenes.scene_path("cornell12"), f"--sky={hdr}", "--w=16",
                            "--h=12", "--samples=6", "--bounces=2", "--hostsim", "--camera=cornell", f"--out={out}",
                            *flags], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    plain, prog, ck = tmp_path / "plain", tmp_path / "prog", tmp_path / "ck"
    run(plain)
    run(prog, "--preview-every=2", f"--checkpoint={tmp_path / 'frame.ckpt'}")
    assert sorted(p.name for p in prog.glob("RT_preview_*.png")) == [f"RT_preview_{d}.png" for d in (2, 4, 6)]
    assert not list(plain.glob("RT_preview_*.png"))
    for n in names:
        assert (prog / n).read_bytes() == (plain / n).read_bytes(), n
    assert (prog / "RT_preview_6.png").read_bytes() == (plain / names[0]).read_bytes()
    assert (prog / "RT_preview_2.png").read_bytes() != (plain / names[0]).read_bytes()
    assert "Resuming" in run(ck, f"--checkpoint={tmp_path / 'frame.ckpt'}")
    assert (ck / names[0]).read_bytes() == (plain / names[0]).read_bytes()
