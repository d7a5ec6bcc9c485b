"""Adaptive progressions on the hostsim build (the same source as the gfx950 kernels' arithmetic, compiled for
the CPU): the cases of tests/adapt_cases.py. The selection is held to a numpy restatement, the rendered pixels
to the untracked uniform progression and the oracle."""
from __future__ import annotations

import pytest

import adapt_cases as ac


@pytest.mark.parametrize("which", ["zero", "median", "above"])
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_selection_by_injected_state(shape, which):
    ac.case_select(True, shape, which)


@pytest.mark.parametrize("scene,step,off,stride", [("cornell", 2, 0, 1), ("fan", 2, 0, 1), ("cornell", 1, 0, 1),
                                                   ("cornell", 2, 1, 3)], ids=["cornell", "fan", "step1", "shard"])
def test_chain_identity_fold_and_noise(scene, step, off, stride):
    ac.case_chain(True, scene, step, off, stride)


def test_checkpoint():
    ac.case_checkpoint(True)


def test_errors_and_state():
    ac.case_errors(True)


def test_python_render_kernel():
    ac.case_python(True)


def _png_rgba(path, w, h):
    """An 8-bit RGBA (or RGB) PNG without interlace as [h, w, 4] uint8: zlib and the five row filters."""
    import struct
    import zlib

    import numpy as np

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, idat, head = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    assert head[:2] == (w, h) and head[2] == 8 and head[3] in (2, 6) and head[6] == 0, head
    bpp = 4 if head[3] == 6 else 3
    raw = zlib.decompress(idat)
    rows = np.zeros((h + 1, w * bpp), np.int32)
    for y in range(h):
        f, line = raw[y * (w * bpp + 1)], np.frombuffer(raw[y * (w * bpp + 1) + 1:(y + 1) * (w * bpp + 1)], np.uint8).astype(np.int32)
        up = rows[y]
        cur = rows[y + 1]
        for i in range(w * bpp):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            b = up[i]
            pa, pb, pc_ = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc_ else (b if pb <= pc_ else c))[f]
            cur[i] = (line[i] + pred) & 255
    out = rows[1:].reshape(h, w, bpp).astype(np.uint8)
    if bpp == 3:
        out = np.concatenate([out, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return out


def test_cli_adaptive(tmp_path):
    """--adaptive at threshold 0 takes every tile in every pass: the four PNGs of a run without flags, byte for
    byte, and a white sample-count map; at a threshold above every tile error the run stops after the two
    uniform passes with a map at 2 / 4; the flag needs --noise-threshold."""
    import os
    import subprocess
    import sys

    import numpy as np

    import rt_amd
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

    plain, full, early, bad = (tmp_path / n for n in ("plain", "full", "early", "bad"))
    run(plain)
    out = run(full, "--preview-every=1", "--noise-threshold=0", "--adaptive")
    assert out.count("adaptive: ") == 4 and "adaptive: 4 of 4 tiles, counts 4 .. 4, capped 0" in out, out
    for n in names:
        assert (full / n).read_bytes() == (plain / n).read_bytes(), n
    assert (_png_rgba(full / "RT_samples.png", w, h) == 255).all(), "every tile at the total: a white map"
    out = run(early, "--preview-every=1", "--noise-threshold=1e30", "--adaptive")
    assert out.count("adaptive: ") == 2, out
    px = _png_rgba(early / "RT_samples.png", w, h)
    half = int(rt_amd.image_to_rgba8(rt_amd.Image.from_rgb(np.full((1, 1, 3), 0.5, np.float32)))[0, 0, 0])
    assert 100 < half < 160 and (px[..., :3] == half).all() and (px[..., 3] == 255).all(), f"2 of 4 samples in grey: {px[0, 0]}"
    assert sorted(p.name for p in early.glob("*.png")) == sorted(names + ["RT_samples.png", "RT_preview_1.png", "RT_preview_2.png"])
    assert (early / "RT_samples.png").read_bytes() != (full / "RT_samples.png").read_bytes()
    run(bad, "--preview-every=1", "--adaptive", code=2)
