"""python -m rt_amd.cli [obj] --sky= --w= --h= --samples= --bounces=

The reference's command line (source/main.cpp:32-61, same flags and defaults) over the
product library: ingest, RenderKernel.render(), the denoise stage at blend 1.0 / 0.75 / 0.5
(main.cpp:118-120) and the four PNGs (main.cpp:122-125). Also --camera=<preset> (default
the dragon camera, main.cpp:110), --out=<directory> (default .) and --hostsim (the CPU
build of the device code, for machines without a GPU). The filter runs once; the three
images are blends of its output with the render (utils.cpp:184-186).

Progressive rendering (RenderKernel.progress_*): --preview-every=K renders in passes of K samples
and writes RT_preview_<done>.png after each (a preview is the mean of the first `done` samples of
the --samples chain, not the frame --samples=<done> gives); --checkpoint=PATH saves the progression
after each pass and resumes from PATH when it exists (same scene, sky, camera and size: the file
does not fingerprint them). The four PNGs at the end are the same as without these flags.

Display stage (RenderKernel.render_linear / display): --exposure=E and --gamma=G tone-map with the
caller's parameters instead of the reference's 1.5 and 2.2, and --hdr-out=PATH writes the linear
radiance as a Radiance .hdr file. With any of the three the frame is rendered linear (or resolved
linear at the end of a progression), written to --hdr-out, then displayed; the denoise stage and the
four PNGs follow as before, and previews are displayed with the same parameters. --exposure=1.5
--gamma=2.2 writes the bytes of a run without flags; with none of the three the run takes the
tone-mapped render's path unchanged.

Noise estimate (RenderKernel.progress_track_noise / progress_noise): --noise-threshold=T, with
--preview-every=K, tracks the progression, and from the second pass on prints one line per pass
(done, max_tile, tiles_over) and stops the passes once no 8x8 tile's error is above T. The four PNGs
(and --hdr-out) then come from the samples done so far. A progression resumed from an untracked
--checkpoint stays untracked and runs to the end. Without the flag a run writes the bytes it writes today.

Adaptive sampling (RenderKernel.progress_advance_adaptive): --adaptive, with --noise-threshold=T and
--preview-every=K. After two uniform passes every further pass advances only the 8x8 tiles whose error
is still above T, until none is (or none fits under --samples any more: keep --samples a multiple of K).
It also writes a fifth PNG, RT_samples.png: tile_n / samples in grey, so that one sees where the samples
went. Without --adaptive nothing changes.

Variance-guided denoise (RenderKernel.denoise_var): --denoise=var, with --noise-threshold=T. The frame is
resolved linear, filtered with the progression's own per-pixel noise figure (progress_noise_sigma) as the
colour edge-stop's scale, and then displayed; the three denoised PNGs are blends of that image with the
render instead of the fixed-sigma filter's. It needs a tracked progression of at least two passes.
--denoise=atrous (the default) is the run without the flag, byte for byte.

Firefly rejection (RenderKernel.firefly_clamp): --firefly or --firefly=GAIN, with --denoise=var only. The linear
frame and its noise figure pass through rt_firefly (its defaults, or GAIN in the place of the default gain) between
the resolve and the filter, and the line "firefly: clamped N of M pixels" is printed. RT_output.png and --hdr-out
stay the unclamped render; the three denoised PNGs come from the clamped frame. Without the flag a run writes the
bytes it writes today.

Exposure metering (RenderKernel.auto_exposure): --auto-exposure or --auto-exposure=KEY, not with --exposure=. The
run goes through render_linear and display as with --gamma=; the final linear frame (under --denoise=var the
filtered one) is metered, the line "auto-exposure: E" is printed and the frame is displayed with E instead of 1.5.
KEY replaces the default key of 0.18. Each preview is metered on its own. Without the flag a run writes the bytes
it writes today.

Guided upscale (RenderKernel.upscale): --upscale=F, 1 < F <= 4. The scene is rendered, and under --denoise=var
filtered, at max(1, round(w / F)) x max(1, round(h / F)); the first-hit guides are rendered at that size and at
w x h, the linear frame (and the filtered one) is upscaled along them, and metering, display, --hdr-out, the
fixed-sigma filter and the four PNGs follow at w x h. The run goes through render_linear and display as with
--gamma=. Previews, checkpoints and RT_samples.png have the low size. The line "upscale: WLxHL -> WxH" is printed.
Without the flag a run writes the bytes it writes today.

Bloom (RenderKernel.bloom): --bloom or --bloom=INTENSITY. The run goes through render_linear and display as with
--gamma=. The frame that would be displayed (under --denoise=var the filtered one as well) is metered first, so that
--auto-exposure does not chase the glow, then passes through rt_bloom (its defaults, or INTENSITY in the place of the
default intensity), then is displayed; the line "bloom: N levels, M of P pixels above threshold" is printed. --hdr-out
stays the frame before bloom, and previews are not bloomed. Without the flag a run writes the bytes it writes today.

Depth of field (RenderKernel.dof): --dof or --dof=COC_INF, with --focus=T or --focus-at=X,Y (default: the centre
pixel). The run goes through render_linear and display as with --gamma=. The linear frame (under --denoise=var the
filtered one as well), after --upscale= if given, passes through rt_dof along the first-hit distances of the guides at
its size (--guides=), before it is metered, bloomed and displayed: its defaults, or COC_INF in the place of the
default coc_inf; the focus distance is T, or rt_amd.focus_at at pixel X,Y. The line "dof: focus T, coc_inf C,
max_radius R, largest radius M" is printed. --hdr-out stays the frame before the blur, and previews are sharp.
--dof=0 writes the bytes of a run without the flag. Under --denoise=var the variance-guided filter runs first, on
the sharp frame with its pinhole guides, and the lens blurs its result. Under the default --denoise=atrous the three
RT_output_denoised_* files are, as with --bloom, the a-trous filter applied to the displayed frame, here the blurred
one, with the pinhole guides: the filter's edge-stops then follow the sharp geometry and not the blurred image, so
those three files are not a filtered lens image in the sense above; RT_output.png is.

Motion blur (RenderKernel.motion_vectors, RenderKernel.motion_blur): --motion-blur or --motion-blur=SHUTTER, with
--prev-camera=PRESET, the camera of the frame before this one (the presets of --camera=). The run goes through
render_linear and display as with --gamma=. The linear frame (under --denoise=var the filtered one as well), after
--upscale= and --dof if given, passes through rt_motion_blur along the vectors rt_motion_vectors gives for the guides
at its size and the previous camera, before it is metered, bloomed and displayed: its defaults, or SHUTTER in the place
of the default shutter. The line "motion blur: shutter S, max_radius R, longest reach M" is printed. --hdr-out stays
the sharp frame, previews are sharp, and --motion-blur=0 writes the bytes of a run without the flag. What --dof says
about the three RT_output_denoised_* files under the default --denoise=atrous holds here too.

Guide source (RenderKernel.guide_source): --guides=walks|exact, default exact. exact takes the first-hit guides of the
filters and of --upscale= from features(), as a run without the flag does, byte for byte; walks takes them from
gbuffer(), the render's own search-BVH walks with the 8-lane exact walk behind them.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

import rt_amd


def parse(argv):
    a = dict(obj="data/OBJs/cornell_pbr.obj", sky="data/Skyspheres/evening_road_01_puresky_2k.hdr", w=512, h=512,
             samples=64, bounces=8, camera="dragon", out=".", hostsim=False, preview_every=0, checkpoint="",
             exposure=None, gamma=None, hdr_out="", noise_threshold=None, adaptive=False, denoise="atrous", firefly=None,
             auto_exposure=None, upscale=None, guides="exact", bloom=None, dof=None, focus=None, focus_at=None,
             motion_blur=None, prev_camera=None)
    for s in argv:
        if s == "--hostsim":
            a["hostsim"] = True
        elif s == "--adaptive":
            a["adaptive"] = True
        elif s == "--firefly":  # (the stage's default gain)
            a["firefly"] = {}
        elif s.startswith("--firefly="):
            a["firefly"] = {"gain": float(s.split("=", 1)[1])}
        elif s == "--bloom":  # (the stage's default intensity)
            a["bloom"] = {}
        elif s.startswith("--bloom="):
            a["bloom"] = {"intensity": float(s.split("=", 1)[1])}
        elif s == "--dof":  # (the stage's default coc_inf)
            a["dof"] = {}
        elif s.startswith("--dof="):
            a["dof"] = {"coc_inf": float(s.split("=", 1)[1])}
        elif s == "--motion-blur":  # (the stage's default shutter)
            a["motion_blur"] = {}
        elif s.startswith("--motion-blur="):
            a["motion_blur"] = {"shutter": float(s.split("=", 1)[1])}
        elif s.startswith("--focus-at="):
            try:
                a["focus_at"] = tuple(int(v) for v in s.split("=", 1)[1].split(","))
            except ValueError:  # (not integers: main() refuses a tuple that is not a pixel)
                a["focus_at"] = ()
        elif s == "--auto-exposure":  # (the solve's default key)
            a["auto_exposure"] = {}
        elif s.startswith("--auto-exposure="):
            a["auto_exposure"] = {"key": float(s.split("=", 1)[1])}
        elif s.startswith(("--sky=", "--camera=", "--out=", "--checkpoint=", "--hdr-out=", "--denoise=", "--guides=", "--prev-camera=")):
            k, v = s[2:].split("=", 1)
            a[k.replace("-", "_")] = v
        elif s.startswith(("--exposure=", "--gamma=", "--noise-threshold=", "--upscale=", "--focus=")):
            k, v = s[2:].split("=", 1)
            a[k.replace("-", "_")] = float(v)
        elif s.startswith(("--w=", "--h=", "--samples=", "--bounces=", "--preview-every=")):
            k, v = s[2:].split("=", 1)
            a[k.replace("-", "_")] = int(v)
        else:
            a["obj"] = s  # (assuming the OBJ file path, as main.cpp:57-59)
    return a


def blend(filtered: rt_amd.Image, image: rt_amd.Image, factor: float) -> rt_amd.Image:
    """utils.cpp:184-186 in float32: factor * filtered + (1 - factor) * image, alpha 1."""
    f = np.float32(factor)
    out = rt_amd.Image(image.width, image.height)
    out.pixels[..., :3] = f * filtered.pixels[..., :3] + (np.float32(1.0) - f) * image.pixels[..., :3]
    out.pixels[..., 3] = 1.0
    return out


def display_stage(a: dict) -> bool:
    """Any of --exposure, --gamma, --hdr-out, --auto-exposure: the run goes through render_linear and display."""
    return a["exposure"] is not None or a["gamma"] is not None or bool(a["hdr_out"]) or a["auto_exposure"] is not None


def linear_path(a: dict) -> bool:
    """The frame is rendered or resolved linear and displayed afterwards: the display stage's flags,
    --denoise=var, which filters the linear frame, --upscale=, which upscales it, --dof or --motion-blur, which blur it, or
    --bloom, which adds its glow."""
    return (display_stage(a) or a["denoise"] == "var" or a["upscale"] is not None or a["bloom"] is not None
            or a["dof"] is not None or a["motion_blur"] is not None)


def low_size(a: dict):
    """--upscale=F: the size the scene is rendered at."""
    return max(1, int(round(a["w"] / a["upscale"]))), max(1, int(round(a["h"] / a["upscale"])))


def display_args(a: dict, exposure=None) -> dict:
    """exposure: the metered one of --auto-exposure, in the place of --exposure= or 1.5."""
    if exposure is None:
        exposure = 1.5 if a["exposure"] is None else a["exposure"]
    return dict(exposure=exposure, gamma=2.2 if a["gamma"] is None else a["gamma"])


def metered(rk: rt_amd.RenderKernel, linear: rt_amd.Image, a: dict, what: str = ""):
    """--auto-exposure: the exposure RenderKernel.auto_exposure gives for this frame, printed; else None."""
    if a["auto_exposure"] is None:
        return None
    e = rk.auto_exposure(linear, **a["auto_exposure"])
    print(f"auto-exposure{what}: {e:.9g}")
    return e


def bloomed(rk: rt_amd.RenderKernel, linear: rt_amd.Image, a: dict, say: bool = True) -> rt_amd.Image:
    """--bloom: the frame through RenderKernel.bloom, with its line printed (say); else the frame itself."""
    if a["bloom"] is None:
        return linear
    p = rt_amd._params(rk.L, rt_amd.BloomParams, "bloom", a["bloom"])
    c = linear.pixels
    with np.errstate(all="ignore"):  # (rt_firefly's luminance in float32, as the stage computes it)
        lum = (np.float32(0.2126) * c[..., 0] + np.float32(0.7152) * c[..., 1]) + np.float32(0.0722) * c[..., 2]
        above = int((lum > np.float32(p.threshold)).sum())
    if say:
        print(f"bloom: {p.levels} levels, {above} of {lum.size} pixels above threshold")
    return rk.bloom(linear, params=p)


def dof_setup(rk: rt_amd.RenderKernel, a: dict, size, guides):
    """--dof: (normal_depth at `size`, the stage's parameters with the focus of --focus= or --focus-at=), with its
    line printed; else None. guides: the (albedo, normal_depth) pair at `size` if the run has it already."""
    if a["dof"] is None:
        return None
    nd = (guides if isinstance(guides, tuple) else rk.guides(size=size))[1]
    p = rt_amd._params(rk.L, rt_amd.DofParams, "dof", a["dof"])
    if a["focus"] is not None:
        p.focus = a["focus"]
    else:
        x, y = a["focus_at"] if a["focus_at"] is not None else (size[0] // 2, size[1] // 2)
        p.focus = rt_amd.focus_at(nd, x, y)
    return nd, p


def dof_blurred(rk: rt_amd.RenderKernel, linear: rt_amd.Image, setup, say: bool = True) -> rt_amd.Image:
    """--dof: the frame through RenderKernel.dof, with its line printed (say); else the frame itself."""
    if setup is None:
        return linear
    nd, p = setup
    out, radius = rk.dof(linear, nd, p, coc=True)
    if say:
        print(f"dof: focus {p.focus:.9g}, coc_inf {p.coc_inf:.9g}, max_radius {p.max_radius}, largest radius {radius.max():.9g}")
    return out


def motion_setup(rk: rt_amd.RenderKernel, a: dict, size, guides):
    """--motion-blur: (normal_depth at `size`, the vectors against --prev-camera=, the stage's parameters); else None.
    guides: the (albedo, normal_depth) pair at `size` if the run has it already."""
    if a["motion_blur"] is None:
        return None
    nd = (guides if isinstance(guides, tuple) else rk.guides(size=size))[1]
    p = rt_amd._params(rk.L, rt_amd.MotionParams, "motion", a["motion_blur"])
    return nd, rk.motion_vectors(nd, rt_amd.Camera.preset(a["prev_camera"])), p


def motion_blurred(rk: rt_amd.RenderKernel, linear: rt_amd.Image, setup, say: bool = True) -> rt_amd.Image:
    """--motion-blur: the frame through RenderKernel.motion_blur, with its line printed (say); else the frame itself."""
    if setup is None:
        return linear
    nd, motion, p = setup
    out, reach = rk.motion_blur(linear, nd, motion, p, reach=True)
    if say:
        print(f"motion blur: shutter {p.shutter:.9g}, max_radius {p.max_radius}, longest reach {reach.max():.9g}")
    return out


def render_progressive(rk: rt_amd.RenderKernel, fb: rt_amd.Image, a: dict):
    """The frame in passes: previews and / or a checkpoint after each; fb ends as render() leaves it
    (display stage or --denoise=var: as render_linear() leaves it). Returns the linear frame filtered by
    denoise_var under --denoise=var, else None."""
    step = a["preview_every"] if a["preview_every"] > 0 else a["samples"]
    ck = a["checkpoint"]
    if ck and os.path.exists(ck):
        with open(ck, "rb") as f:
            rk.progress_load(f.read())
        print(f"Resuming {ck} at {rk.progress_info()['done']} samples")
    else:
        rk.progress_begin()
        if a["noise_threshold"] is not None:
            rk.progress_track_noise()
    os.makedirs(a["out"], exist_ok=True)
    passes = 0
    preview = rt_amd.Image(a["w"], a["h"])
    while True:
        i = rk.progress_info()
        if i["done"] >= i["total"]:
            break
        if a["adaptive"]:  # (the first two passes take every tile: there is no estimate yet)
            n = rk.progress_advance_adaptive(step, a["noise_threshold"])
            if n["active_tiles"] == 0:
                break
            done = (passes + 1) * step  # (previews are named by the samples a tile active in every pass has)
            print(f"adaptive: {n['active_tiles']} of {n['tiles']} tiles, counts {n['min_count']} .. {n['max_count']}, "
                  f"capped {n['capped_tiles']}")
        else:
            done = rk.progress_advance(step)
        if ck:
            with open(ck + ".tmp", "wb") as f:
                f.write(rk.progress_save())
            os.replace(ck + ".tmp", ck)
        if a["preview_every"] > 0:
            if display_stage(a):
                rk.progress_resolve_linear(preview)
                shown = rk.display(preview, **display_args(a, metered(rk, preview, a, f" (preview {done})")))
            else:
                shown = rk.progress_resolve(preview)
            rt_amd.write_image_png(shown, os.path.join(a["out"], f"RT_preview_{done}.png"))
        passes += 1
        if a["adaptive"]:  # (an adaptive pass that finds no tile above the threshold ends the loop)
            continue
        if a["noise_threshold"] is not None and passes >= 2:
            try:
                n = rk.progress_noise(a["noise_threshold"])
            except rt_amd.RtError:  # (resumed from an untracked checkpoint, or one pass into a tracked one)
                continue
            print(f"noise: done {done} max_tile {n['max_tile']:.6g} tiles_over {n['tiles_over']}")
            if n["tiles_over"] == 0:
                break
    filtered = None
    if linear_path(a):
        rk.progress_resolve_linear(fb)
        if a["denoise"] == "var":  # (the sigma of the live progression, then the filter on the linear frame)
            with np.errstate(all="ignore"):
                if a["firefly"] is None:
                    filtered = rk.denoise_var(fb, None, 1.0)
                else:  # (the clamp scales the noise figure with the colour: the filter takes both)
                    clamped, sigma, scale = rk.firefly_clamp(fb, rk.progress_noise_sigma(), a["firefly"], return_scale=True)
                    print(f"firefly: clamped {int((scale < 1).sum())} of {scale.size} pixels")
                    filtered = rk.denoise_var(clamped, sigma, 1.0)
    else:
        rk.progress_resolve(fb)
    if a["adaptive"]:  # where the samples went: tile_n / total in grey
        tile_n, _ = rk.progress_tile_counts()
        grey = np.repeat(np.repeat(tile_n, 8, 0), 8, 1)[:a["h"], :a["w"]].astype(np.float32) / np.float32(a["samples"])
        counts = rt_amd.Image(a["w"], a["h"])
        counts.pixels[..., :3] = grey[..., None]
        counts.pixels[..., 3] = 1.0
        rt_amd.write_image_png(counts, os.path.join(a["out"], "RT_samples.png"))
    rk.progress_end()
    return filtered


def main(argv=None) -> int:
    a = parse(sys.argv[1:] if argv is None else argv)
    if a["noise_threshold"] is not None and a["preview_every"] <= 0:
        print("--noise-threshold needs --preview-every=K (the estimate compares passes)", file=sys.stderr)
        return 2
    if a["adaptive"] and a["noise_threshold"] is None:
        print("--adaptive needs --noise-threshold=T and --preview-every=K", file=sys.stderr)
        return 2
    if a["denoise"] not in ("atrous", "var"):
        print("--denoise= takes atrous or var", file=sys.stderr)
        return 2
    if a["guides"] not in ("walks", "exact"):
        print("--guides= takes walks or exact", file=sys.stderr)
        return 2
    if a["denoise"] == "var" and a["noise_threshold"] is None:
        print("--denoise=var needs --noise-threshold=T and --preview-every=K (it filters with the progression's "
              "noise estimate)", file=sys.stderr)
        return 2
    if a["firefly"] is not None and a["denoise"] != "var":
        print("--firefly needs --denoise=var (it clamps the linear frame the variance-guided filter takes)", file=sys.stderr)
        return 2
    if a["firefly"] and not a["firefly"]["gain"] >= 0.0:
        print("--firefly=GAIN takes a gain of at least 0", file=sys.stderr)
        return 2
    if a["auto_exposure"] is not None and a["exposure"] is not None:
        print("--auto-exposure meters the exposure: it does not go with --exposure=", file=sys.stderr)
        return 2
    if a["auto_exposure"] and not 0.0 < a["auto_exposure"]["key"] < 1.0:
        print("--auto-exposure=KEY takes a key inside (0, 1)", file=sys.stderr)
        return 2
    if a["bloom"] and not (0.0 <= a["bloom"]["intensity"] < float("inf")):
        print("--bloom=INTENSITY takes a finite intensity of at least 0", file=sys.stderr)
        return 2
    if a["dof"] and not (0.0 <= a["dof"]["coc_inf"] < float("inf")):
        print("--dof=COC_INF takes a finite radius in pixels of at least 0", file=sys.stderr)
        return 2
    if (a["focus"] is not None or a["focus_at"] is not None) and a["dof"] is None:
        print("--focus= and --focus-at= need --dof", file=sys.stderr)
        return 2
    if a["focus"] is not None and a["focus_at"] is not None:
        print("--focus=T and --focus-at=X,Y do not go together", file=sys.stderr)
        return 2
    if a["focus"] is not None and not (0.0 < a["focus"] < float("inf")):
        print("--focus=T takes a finite distance above 0", file=sys.stderr)
        return 2
    if a["focus_at"] is not None and (len(a["focus_at"]) != 2 or not (0 <= a["focus_at"][0] < a["w"] and 0 <= a["focus_at"][1] < a["h"])):
        print("--focus-at=X,Y takes a pixel of the frame", file=sys.stderr)
        return 2
    if a["motion_blur"] and not (0.0 <= a["motion_blur"]["shutter"] <= 1.0):
        print("--motion-blur=SHUTTER takes a share of the frame interval inside [0, 1]", file=sys.stderr)
        return 2
    if a["prev_camera"] is not None and a["motion_blur"] is None:
        print("--prev-camera= needs --motion-blur", file=sys.stderr)
        return 2
    if a["motion_blur"] is not None:
        try:
            rt_amd.Camera.preset(a["prev_camera"])
        except Exception:  # (no preset of that name, or none given)
            print("--motion-blur needs --prev-camera=PRESET, a camera preset as --camera= takes", file=sys.stderr)
            return 2
    if a["upscale"] is not None and not 1.0 < a["upscale"] <= 4.0:
        print("--upscale=F takes a factor with 1 < F <= 4", file=sys.stderr)
        return 2
    print(f"Reading OBJ {a['obj']} ...")
    P = rt_amd.parse_obj(a["obj"])
    print(f"Reading Environment Map {a['sky']} ...")
    sky = rt_amd.read_image_float(a["sky"])
    print(f"[{a['w']}x{a['h']}]: {a['samples']} samples\n")
    t0 = time.perf_counter()
    full = (a["w"], a["h"])
    if a["upscale"] is not None:  # (everything up to the upscale runs at the low size)
        a = dict(a, w=low_size(a)[0], h=low_size(a)[1])
    fb = rt_amd.Image(a["w"], a["h"])
    rk = rt_amd.RenderKernel(a["w"], a["h"], a["samples"], a["bounces"], fb, P.triangles, P.materials,
                             P.emissive_triangle_indices, P.material_indices, None, rt_amd.BVH(P.triangles), sky,
                             rt_amd.compute_env_map_cdf(sky), hostsim=a["hostsim"])
    rk.set_camera(rt_amd.Camera.preset(a["camera"]))
    rk.guide_source = a["guides"]
    filtered = None
    if a["preview_every"] > 0 or a["checkpoint"]:
        try:
            filtered = render_progressive(rk, fb, a)
        except rt_amd.RtError as e:
            if a["denoise"] != "var" or "rt_progress_noise_sigma" not in str(e):
                raise
            print(f"--denoise=var: {e}", file=sys.stderr)
            return 2
    elif linear_path(a):
        rk.render_linear()
    else:
        rk.render()
    guides = True
    if a["upscale"] is not None:  # (the linear frame, and the filtered one, to the full size along the guides)
        print(f"upscale: {a['w']}x{a['h']} -> {full[0]}x{full[1]}")
        low_guides, guides = rk.guides(), rk.guides(size=full)
        fb = rk.upscale(fb, *low_guides, *guides)
        if filtered is not None:
            filtered = rk.upscale(filtered, *low_guides, *guides)
    if linear_path(a):  # fb holds the linear radiance: the .hdr file, then the displayed frame
        if a["hdr_out"]:
            rt_amd.write_image_hdr(fb, a["hdr_out"])
        try:
            lens = dof_setup(rk, a, full, guides)
        except ValueError as e:  # (focus_at on a frame without a hit)
            print(f"--dof: {e}", file=sys.stderr)
            return 2
        fb = dof_blurred(rk, fb, lens)
        if filtered is not None:
            filtered = dof_blurred(rk, filtered, lens, say=False)
        shutter = motion_setup(rk, a, full, guides)
        fb = motion_blurred(rk, fb, shutter)
        if filtered is not None:
            filtered = motion_blurred(rk, filtered, shutter, say=False)
        args = display_args(a, metered(rk, fb if filtered is None else filtered, a))
        fb = rk.display(bloomed(rk, fb, a), **args)
        if filtered is not None:
            filtered = rk.display(bloomed(rk, filtered, a, say=False), **args)
    print(f"{int((time.perf_counter() - t0) * 1e3)}ms")
    with np.errstate(all="ignore"):
        if filtered is None:
            filtered = rk.denoise(fb, 1.0, guides)
        os.makedirs(a["out"], exist_ok=True)
        rt_amd.write_image_png(fb, os.path.join(a["out"], "RT_output.png"))
        for factor, name in ((1.0, "1"), (0.75, "0.75"), (0.5, "0.5")):
            rt_amd.write_image_png(blend(filtered, fb, factor), os.path.join(a["out"], f"RT_output_denoised_{name}.png"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
