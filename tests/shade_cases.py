"""The shading zoo: env maps at every size where the env-CDF search changes form or indexing
(rt_trace.h cdf_search: fence tables in LDS, fence tables in global memory, the reference's binary
search) with contents that make flat runs, a zero total, a decreasing CDF, inf and NaN; material
tables and emissive lists outside what the scenes' MTL files hold; and framebuffers that are not
zero on entry. One geometry (the 12-triangle Cornell box, plus one zero-area triangle for the
degenerate light), one frame size. Shared by tests/test_shade.py (oracle, hostsim),
tests/test_shade_gpu.py (gfx950) and tools/gen_golden_shade.py (the reference's frames,
tests/golden/shade_*.npz).

Pure numpy: every array comes from a seeded generator or a fixed formula and is float32."""
from __future__ import annotations

import os
from collections import OrderedDict, namedtuple

import numpy as np

FRAME = dict(W=48, H=36, spp=4, bounces=4)
SEED = 7100
LDS_ROWS = 1024  # rt_trace.h RT_CDF_LDS_ROWS

Case = namedtuple("Case", "name zoo env mats em fb flag")

# ---------------------------------------------------------------- the env zoo
# (w, h): what the size reaches is in the issue's table (tests/test_shade.py asserts the forms)
ENV_SIZES = [(1, 1), (1, 8), (16, 1), (48, 7), (20, 9), (127, 5), (16, 1024), (16, 1025), (16, 1040), (16, 4097),
             (16, 4098), (4096, 2), (4112, 2)]
# one size per search form, crossed with every content
FORM_SIZES = [(48, 7), (16, 1040), (20, 9)]
CONTENTS = ["grad", "black60", "first", "last", "black", "neg", "inf", "nan", "rgba"]
ENVS = [f"grad_{w}x{h}" for w, h in ENV_SIZES] + [f"{c}_{w}x{h}" for c in CONTENTS[1:] for w, h in FORM_SIZES]

_envs: dict = {}


def _grad(w, h):
    """A vertical gradient and a bright block, as scenes.make_sky."""
    s = (np.arange(h, dtype=np.float32)[:, None] / np.float32(h)) * np.ones((1, w), np.float32)
    img = np.empty((h, w, 3), np.float32)
    img[..., 0] = np.float32(0.3) + np.float32(0.5) * s
    img[..., 1] = np.float32(0.4) + np.float32(0.4) * s
    img[..., 2] = np.float32(0.6) + np.float32(0.4) * s
    n = max(1, min(w, h) // 8)
    y0, x0 = (3 * h) // 4, (5 * w) // 8
    img[y0:y0 + n, x0:x0 + n] = np.float32([200.0, 180.0, 150.0])
    return img


def env(name: str) -> np.ndarray:
    """[h, w, 3] float32, or [h, w, 4] for the content "rgba" (junk in alpha); "S": the suite's sky."""
    if name in _envs:
        return _envs[name]
    if name == "S":
        import rt_cases
        img = rt_cases.sky("S")
    else:
        content, size = name.split("_")
        w, h = (int(v) for v in size.split("x"))
        rng = np.random.default_rng([SEED, CONTENTS.index(content), w, h])
        img = _grad(w, h)
        mid = ((h // 2) * w + w // 3)
        flat = img.reshape(-1, 3)
        if content == "black60":
            flat[rng.random(w * h) < 0.6] = 0.0
            img[0], img[-1], img[:, 0], img[:, -1] = 0.0, 0.0, 0.0, 0.0
        elif content in ("first", "last"):
            flat[...] = 0.0
            flat[0 if content == "first" else -1] = np.float32([50.0, 40.0, 30.0])
        elif content == "black":
            flat[...] = 0.0
        elif content == "neg":
            flat[mid] = np.float32([-5.0, -5.0, -5.0])
        elif content == "inf":
            flat[mid, 1] = np.inf
        elif content == "nan":
            flat[mid, 2] = np.nan
        elif content == "rgba":
            a = rng.uniform(-1e30, 1e30, (h, w, 1)).astype(np.float32)
            a.reshape(-1)[::5] = np.nan
            a.reshape(-1)[1::7] = np.inf
            img = np.concatenate([img, a], -1)
    img = np.ascontiguousarray(img, np.float32)
    img.setflags(write=False)
    _envs[name] = img
    return img


def env_cdf(img: np.ndarray) -> np.ndarray:
    """Utils::compute_env_map_cdf (utils.cpp:126-142) over Image::luminance_of_pixel
    (image.h:80-85): the luminance in double rounded to float, summed in float in texel order."""
    c = img[..., :3].reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        lum = (0.3086 * c[:, 0] + 0.6094 * c[:, 1] + 0.0820 * c[:, 2]).astype(np.float32)
        return np.cumsum(lum, dtype=np.float32)


def expected_form(img: np.ndarray) -> str:
    """rt_scene.cpp env_cdf_fences' rule, restated: "lds" / "global" fence search, or "binary"."""
    h, w = img.shape[:2]
    cdf = env_cdf(img)
    if w % 16 != 0 or w - 1 > 4096 or h - 1 > 4096:
        return "binary"
    with np.errstate(invalid="ignore"):
        if np.isnan(cdf).any() or not (cdf[1:] >= cdf[:-1]).all():
            return "binary"
    return "lds" if h <= LDS_ROWS else "global"


def ref_search(img: np.ndarray, values: np.ndarray) -> np.ndarray:
    """RenderKernel::env_map_cdf_search (render_kernel.cpp:532-567) for every value at once:
    [n, 2] int32 = x, y. `value < cdf[i]` is false for a NaN on either side, as in C."""
    h, w = img.shape[:2]
    cdf = env_cdf(img).reshape(h, w)
    v = np.asarray(values, np.float32)
    n = v.shape[0]
    with np.errstate(invalid="ignore"):
        lower, upper = np.zeros(n, np.int64), np.full(n, h - 1, np.int64)
        while True:
            live = lower < upper
            if not live.any():
                break
            mid = (lower + upper) // 2
            lt = v < cdf[np.minimum(mid, h - 1), w - 1]
            upper = np.where(live & lt, mid, upper)
            lower = np.where(live & ~lt, mid + 1, lower)
        y = np.maximum(np.minimum(lower, h), 0)
        lower, upper = np.zeros(n, np.int64), np.full(n, w - 1, np.int64)
        while True:
            live = lower < upper
            if not live.any():
                break
            mid = (lower + upper) // 2
            lt = v < cdf[y, np.minimum(mid, w - 1)]
            upper = np.where(live & lt, mid, upper)
            lower = np.where(live & ~lt, mid + 1, lower)
        x = np.maximum(np.minimum(lower, w), 0)
    return np.stack([x, y], 1).astype(np.int32)


def search_values(img: np.ndarray) -> np.ndarray:
    """The values the search is asked: every distinct CDF entry, its float neighbours for a sample
    of entries, 0, -1, the total and twice it, the infinities, NaN, and 4096 uniform draws."""
    cdf = env_cdf(img)
    rng = np.random.default_rng([SEED, 77, img.shape[0], img.shape[1]])
    ent = np.unique(cdf[~np.isnan(cdf)])
    some = ent[rng.integers(0, ent.shape[0], 512)] if ent.shape[0] else ent
    total = cdf[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        top = np.float32(total if np.isfinite(total) and total > 0 else 1.0)
        draws = (rng.random(4096).astype(np.float32) * top).astype(np.float32)
        special = np.float32([0.0, -0.0, -1.0, total, np.float32(2.0) * total, np.inf, -np.inf, np.nan])
        out = np.concatenate([ent, np.nextafter(some, np.float32(np.inf)), np.nextafter(some, np.float32(-np.inf)),
                              special, draws]).astype(np.float32)
    return np.ascontiguousarray(out)


# ---------------------------------------------------------------- geometry, materials, lights
ZERO_AREA = np.float32([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.3, 1.2, 0.1])  # two equal vertices, inside the box
LIGHT = 5                                                                # cornell12's emitting material
ROUGH, METAL = [0.0, 1e-4, 1.0, 1.5], [0.0, 1.0, -0.25, 1.25]
MATS = (["default"] + [f"r{i}m{j}" for i in range(4) for j in range(4)] +
        ["diffuse15", "black_metal", "emit0", "emit_neg", "emit_nan", "emit_huge"])
EMS = ["default", "empty", "nonemissive", "repeat", "zero_area"]


def _parsed():
    from conftest import parsed_scene
    return parsed_scene("cornell12")


def triangles(em: str = "default") -> np.ndarray:
    t = _parsed().triangles
    return np.ascontiguousarray(np.concatenate([t, ZERO_AREA[None]]) if em == "zero_area" else t, np.float32)


def material_indices(em: str = "default") -> np.ndarray:
    mi = _parsed().material_indices
    return np.concatenate([mi, np.int32([LIGHT])]).astype(np.int32) if em == "zero_area" else mi.copy()


def emissive(em: str = "default") -> np.ndarray:
    lights = _parsed().emissive_triangle_indices  # (2, 3)
    return {"default": lights, "empty": lights[:0], "nonemissive": np.append(lights, 0),
            "repeat": np.int32([lights[0], lights[0], lights[1]]), "zero_area": np.append(lights, 12)}[em].astype(np.int32)


def materials(key: str = "default") -> np.ndarray:
    """[9, 10] float32 over cornell12's material indices."""
    m = _parsed().materials.copy()
    others = (np.arange(m.shape[0]) != LIGHT) & (np.arange(m.shape[0]) != 0)  # (0: parse_obj's default, unused)
    if key[0] == "r" and key[2] == "m":
        m[others, 9], m[others, 8] = np.float32(ROUGH[int(key[1])]), np.float32(METAL[int(key[3])])
    elif key == "diffuse15":
        m[others, 4:7] = 1.5
    elif key == "black_metal":  # the floor and the back wall
        m[[1, 3], 4:7], m[[1, 3], 8] = 0.0, 1.0
    elif key == "emit0":
        m[1:, 0:3] = 0.0
    elif key == "emit_neg":
        m[LIGHT, 0:3] = -100.0
    elif key == "emit_nan":
        m[LIGHT, 1] = np.nan
    elif key == "emit_huge":
        m[LIGHT, 0:3] = 3e38
    elif key != "default":
        raise KeyError(key)
    return m


# ---------------------------------------------------------------- the framebuffer on entry
FBS = ["zero", "random", "negative", "huge", "inf", "nan", "zeros"]


def framebuffer(key: str = "zero") -> np.ndarray:
    """[H, W, 4]: Image's default (0, 0, 0, 1), or the variant. The special values sit on two
    pixels of three, so that each frame keeps pixels that start from zero."""
    W, H = FRAME["W"], FRAME["H"]
    fb = np.zeros((H, W, 4), np.float32)
    fb[..., 3] = 1.0
    rng = np.random.default_rng([SEED, 99, FBS.index(key)])
    k = (np.arange(W)[None, :] + np.arange(H)[:, None]) % 3
    if key == "random":
        fb[..., :3] = rng.uniform(0.0, 2.0, (H, W, 3))
        fb[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    elif key == "negative":
        fb[k == 1, :3] = rng.uniform(-1.0, 0.0, ((k == 1).sum(), 3))
        fb[k == 2, :3] = rng.uniform(-100.0, -1.0, ((k == 2).sum(), 3))
    elif key == "huge":
        fb[k == 1, :3] = 1e30
        fb[k == 2, :3] = -1e30
    elif key == "inf":
        fb[k == 1, :3] = np.inf
        fb[k == 2, :3] = -np.inf
    elif key == "nan":
        fb[k == 1, :3] = np.nan
        fb[k == 2, 1] = np.nan
    elif key == "zeros":
        fb[k == 1, :3] = -0.0
        fb[k == 2, 0:3:2] = -0.0
    return fb


# ---------------------------------------------------------------- the three zoos
# flag: "finite" (no NaN in the oracle's frame, and it shows the scene) or "nan_expected" (some NaN
# pixels, and finite ones that show the scene); tests/test_shade.py asserts each on the oracle
# (a zero total makes the env pdf 0 / 0; a negative texel a negative radiance under the tone map's
# powf where a path samples it, which no path of the 48 x 7 frame does; roughness 0 gives D = 0 and
# 0 / 0 weights except on the pure metal; metalness 1.25 a negative diffuse weight; +-1e30 and +-inf
# on entry tone-map to 1 or +inf, never NaN)
NAN_ENVS = ({f"{c}_{w}x{h}" for c in ("black", "inf", "nan") for w, h in FORM_SIZES} | {"neg_16x1040", "neg_20x9"})
NAN_MATS = {"r0m0", "r0m2", "r0m3", "r1m3", "r3m3", "emit_neg", "emit_nan"}
NAN_FBS = {"negative", "nan"}
ENV_CASES = [Case(f"env-{e}", "env", e, "default", "default", "zero", "nan_expected" if e in NAN_ENVS else "finite")
             for e in ENVS]
MAT_CASES = ([Case(f"mat-{m}", "mat", "S", m, "default", "zero", "nan_expected" if m in NAN_MATS else "finite")
              for m in MATS[1:]] +
             [Case(f"em-{e}", "mat", "S", "default", e, "zero", "finite") for e in EMS[1:]])
FB_CASES = [Case(f"fb-{f}", "fb", "S", "default", "default", f, "nan_expected" if f in NAN_FBS else "finite")
            for f in FBS[1:]]
CASES = ENV_CASES + MAT_CASES + FB_CASES
BY_NAME = {c.name: c for c in CASES}
SKY_ONLY_MIN = 0.1  # tests/test_zoo.py test_frames_see_their_scenes


def camera() -> np.ndarray:
    from conftest import load_golden
    return load_golden("cameras.npz")["cornell"]


_kernels: "OrderedDict" = OrderedDict()
KEEP = 6


def kernel(case: Case, hostsim: bool):
    """A context over the case's scene, sized for FRAME, with its own image (rk.frame_buffer). The
    env goes through rt_set_env with as many channels as the case's array has (3, or 4 for "rgba").
    The last KEEP are cached; tests leave the schedule as they found it."""
    import rt_amd
    from rt_amd import _capi
    key = (case.name, hostsim)
    if key in _kernels:
        _kernels.move_to_end(key)
        return _kernels[key]
    F = FRAME
    tris = triangles(case.em)
    e = env(case.env)
    rk = rt_amd.RenderKernel(F["W"], F["H"], F["spp"], F["bounces"], rt_amd.Image(F["W"], F["H"]), tris,
                             materials(case.mats), emissive(case.em), material_indices(case.em), None, rt_amd.BVH(tris),
                             rt_amd.Image.from_rgb(e), None, hostsim=hostsim)
    _capi.check(rk.L, rk.L.rt_set_env(rk.ctx, _capi.ptr(e), e.shape[1], e.shape[0], e.shape[2], None), rk.ctx, "rt_set_env")
    c = camera()
    rk.set_camera(rt_amd.Camera(c[:16], c[16]))
    _kernels[key] = rk
    while len(_kernels) > KEEP:
        _kernels.popitem(last=False)
    return rk


def render(rk, case: Case) -> np.ndarray:
    """A fresh frame from the case's framebuffer on entry."""
    rk.frame_buffer.pixels[...] = framebuffer(case.fb)
    rk.render()
    return rk.frame_buffer.pixels.copy()


def env_search(rk, form: int, values: np.ndarray) -> np.ndarray:
    """rt_device_env_search: [n, 2] int32 = x, y."""
    from rt_amd import _capi
    v = np.ascontiguousarray(values, np.float32)
    out = np.full((v.shape[0], 2), -7, np.int32)
    _capi.check(rk.L, rk.L.rt_device_env_search(rk.ctx, form, _capi.ptr(v), v.shape[0], _capi.ptr(out)), rk.ctx,
                "rt_device_env_search")
    return out


_oracles: dict = {}
_frames: dict = {}


def oracle(case: Case):
    from oracle_bindings import OracleScene
    key = (case.env, case.mats, case.em)
    if key not in _oracles:
        _oracles[key] = OracleScene(triangles(case.em), material_indices(case.em), materials(case.mats), emissive(case.em),
                                    env=np.ascontiguousarray(env(case.env)[..., :3]))
    return _oracles[key]


def oracle_frame(case: Case) -> np.ndarray:
    """The oracle's frame of the case, computed once and read-only."""
    if case.name not in _frames:
        F = FRAME
        fb, _ = oracle(case).render(camera(), F["W"], F["H"], F["spp"], F["bounces"], fb=framebuffer(case.fb))
        fb.setflags(write=False)
        _frames[case.name] = fb
    return _frames[case.name]


def sky_only_frame(env_name: str) -> np.ndarray:
    """The oracle's frame of the empty scene under the env: what a camera that sees nothing gives."""
    from oracle_bindings import OracleScene
    key = ("sky", env_name)
    if key not in _frames:
        F = FRAME
        S = OracleScene(np.zeros((0, 9), np.float32), np.zeros(0, np.int32), materials(), np.zeros(0, np.int32),
                        env=np.ascontiguousarray(env(env_name)[..., :3]))
        fb, _ = S.render(camera(), F["W"], F["H"], F["spp"], F["bounces"])
        fb.setflags(write=False)
        _frames[key] = fb
    return _frames[key]


# ---------------------------------------------------------------- the scene as OBJ / MTL, the sky as raw
def mtl_expressible(case: Case) -> bool:
    """What Utils::parse_obj (utils.cpp:16-98) can return: roughness max(0.01, Pr), and the
    emissive list is the triangles whose Ke has a positive channel, in order."""
    m = materials(case.mats)
    want = np.flatnonzero((m[material_indices(case.em), 0:3] > 0).any(1))
    return bool((m[1:, 9] >= np.float32(1.0e-2)).all() and np.array_equal(want, emissive(case.em)))


def write_obj(case: Case, directory: str) -> str:
    """shade_<mats>_<em>.obj and .mtl: three vertices per triangle, %.9g."""
    os.makedirs(directory, exist_ok=True)
    stem = f"shade_{case.mats}_{case.em}"
    m, mi, t = materials(case.mats), material_indices(case.em), triangles(case.em)
    with open(os.path.join(directory, stem + ".mtl"), "w") as f:
        for k, r in list(enumerate(m))[1:]:
            f.write("newmtl m%d\nKe %.9g %.9g %.9g\nKd %.9g %.9g %.9g\nillum 1\nPm %.9g\nPr %.9g\n\n" %
                    (k, r[0], r[1], r[2], r[4], r[5], r[6], r[8], r[9]))
    path = os.path.join(directory, stem + ".obj")
    with open(path, "w") as f:
        f.write(f"mtllib {stem}.mtl\no {stem}\n")
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in t.reshape(-1, 3)))
        f.write("".join("usemtl m%d\nf %d %d %d\n" % (mi[i], 3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(t.shape[0])))
    return path


def write_sky_raw(env_name: str, path: str) -> str:
    """The raw file oracle/ref/ref_driver.cpp reads: w, h, then RGB float32."""
    import struct
    e = env(env_name)
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", e.shape[1], e.shape[0]))
        f.write(np.ascontiguousarray(e[..., :3], "<f4").tobytes())
    return path
