"""Golden fixtures for the shading zoo (tests/shade_cases.py), written by the REFERENCE itself
(needs the reference binaries of `make ref`): one 48x36 x 4 spp x 4 bounce frame through
RenderKernel::render per pinned case.

    make ref && python tools/gen_golden_shade.py

Pinned: every env of the zoo (each as the raw RGB sky ref_driver reads) over the default Cornell
box, and the material and emissive-list cases that an OBJ / MTL can express (written under
build/scenes/, vertices and material fields %.9g; the reference's own parse must return the
generator's tables bit for bit). Writes tests/golden/shade_<case>.npz and
tests/golden/shade_manifest.json (data only). A case the reference cannot run is recorded in
the manifest's "unavailable" map with the reason, and only the oracle holds it.
"""
from __future__ import annotations

import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sycl-ray-tracing_amd"))
import golden_io as gio  # noqa: E402
import scenes  # noqa: E402
import shade_cases as sc  # noqa: E402
from gen_golden_brute import run  # noqa: E402

REF = os.path.join(gio.REPO, "oracle", "_ref", "ref_driverO2")
OUT = gio.GOLDEN


def same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed member date, so that a second run writes the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a))
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def main():
    tmp = tempfile.mkdtemp()
    F = sc.FRAME
    man = {"generator": "tools/gen_golden_shade.py", "reference": os.path.relpath(REF, gio.REPO), "frame": F,
           "camera": "cornell", "pinned": {}, "unavailable": {}}
    for case in sc.CASES:
        if case.fb != "zero":
            man["unavailable"][case.name] = "ref_driver renders into a fresh Image: no framebuffer on entry"
            continue
        if not sc.mtl_expressible(case):
            man["unavailable"][case.name] = ("no OBJ / MTL parses to these tables: parse_obj clamps roughness to 0.01 and "
                                             "lists the triangles whose Ke has a positive channel")
            continue
        try:
            obj = sc.write_obj(case, scenes.build_dir())
            run(REF, "parse", obj, os.path.join(tmp, "p.bin"))
            p = gio.read_parse(os.path.join(tmp, "p.bin"))
            if not (same(p["tris"], sc.triangles(case.em)) and np.array_equal(p["mat_idx"], sc.material_indices(case.em)) and
                    np.array_equal(p["emissive"], sc.emissive(case.em)) and same(p["mats"], sc.materials(case.mats))):
                man["unavailable"][case.name] = "the reference's parse of the MTL does not return the tables (a NaN field)"
                continue
            sky = sc.write_sky_raw(case.env, os.path.join(tmp, "sky.raw"))
            out = os.path.join(tmp, "fb.f32")
            run(REF, "render", obj, sky, "cornell", F["W"], F["H"], F["spp"], F["bounces"], out)
        except RuntimeError as e:  # (gen_golden_brute.run: the reference exited non-zero)
            man["unavailable"][case.name] = "the reference exited non-zero on this case"
            print(f"{case.name}: {str(e)[-200:]}", flush=True)
            continue
        rgba = np.fromfile(out, dtype="<f4").reshape(F["H"], F["W"], 4)
        save_npz(os.path.join(OUT, f"shade_{case.name}.npz"), rgba=rgba)
        man["pinned"][case.name] = {"rgba_sha256": gio.sha256(rgba), "nan_pixels": int(np.isnan(rgba[..., :3]).any(-1).sum())}
        print(case.name, man["pinned"][case.name], flush=True)
    for k, v in man["unavailable"].items():
        print("unavailable:", k, "-", v)
    with open(os.path.join(OUT, "shade_manifest.json"), "w") as f:
        json.dump(man, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
