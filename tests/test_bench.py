"""bench.py's command line: --dump-outputs writes what the last timed step returned, a
plain run carries none of the --full objects, and --steps sets the timed steps."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

import bench
import rt_cases


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    rng = np.random.default_rng(5)
    frames = {"a": rng.random((7, 9, 4), dtype=np.float32), "b": rng.random((7, 9, 4), dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "whole"), frames)
    for k, f in frames.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, f)
    # over the budget: the same k pixels of each frame in every run, within the budget in all
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 20 * 16 + 5)
    bench.dump_outputs(str(tmp_path / "s1"), frames)
    bench.dump_outputs(str(tmp_path / "s2"), frames)
    total = 0
    for k, f in frames.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        assert s1.dtype == np.float32 and s1.shape == (20, 4)
        np.testing.assert_array_equal(s1, s2)
        px = f.reshape(-1, 4)
        idx = [int(np.flatnonzero((px == row).all(axis=1))[0]) for row in s1]
        assert idx == sorted(set(idx))  # distinct pixels of the frame, in frame order
        total += s1.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    # `of`: the budget is shared with frames that other ranks write
    bench.dump_outputs(str(tmp_path / "s3"), {"a": frames["a"]}, of=4)
    assert np.load(tmp_path / "s3" / "a.npy").shape == (10, 4)


def test_scene_file_falls_back_when_the_tree_is_read_only(tmp_path, monkeypatch):
    import scenes
    import tempfile
    want = open(scenes.scene_path("cornell12"), "rb").read()

    def denied(name):
        raise PermissionError(13, "Permission denied", os.path.join(scenes.REPO, "build", "scenes"))

    monkeypatch.setattr(scenes, "scene_path", denied)
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    p = bench.scene_file("cornell12")
    assert os.path.dirname(os.path.dirname(p)) == str(tmp_path)
    assert open(p, "rb").read() == want and os.path.exists(os.path.join(os.path.dirname(p), "cornell_pbr.mtl"))
    assert bench.scene_file("cornell12") == p  # (kept for the next run)
    with pytest.raises(PermissionError):
        bench.scene_file("mis")  # (not a CONFIGS scene: no fallback)


@pytest.mark.gpu
def test_gpu_plain_run_dumps_the_timed_frame(manifest, tmp_path, monkeypatch, capsys):
    """cfg1 (the Cfg1 golden's frame) through bench.main: the dumped frame is the compiled
    reference's golden bit for bit, and the line is a plain run's."""
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "cfg1", "--steps", "2", "--warmup", "1",
                                      "--dump-outputs", str(out)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "Msamples/s" and line["higher_is_better"] is True
    # (value and ms_per_step are each rounded to 1e-3)
    assert line["value"] == pytest.approx(256 * 256 * 4 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert line["roofline"] is None and line["cpu_baseline"] is None and line["parity"] is None
    assert "exact_handovers" not in line
    assert os.listdir(out) == ["frame.npy"]
    fb = np.load(out / "frame.npy")
    e = rt_cases.golden_case("cfg1_cornell12", manifest)
    assert fb.dtype == np.float32
    np.testing.assert_array_equal(fb.view(np.uint32), e["expected"].view(np.uint32))
