"""Linear radiance and the display stage (rt_render_linear, rt_progress_resolve_linear, rt_display,
rt_write_hdr; include/rt_hip.h). The strong pin is the round trip: the linear frame pushed through
rt_display at the defaults (1.5, 2.2) is rt_render's frame, and so the oracle's, bit for bit. The
linear frame itself is pinned by numpy float32 arithmetic on a progression's checkpoint, and the
display arithmetic by a float64 model and, on the GPU, by the hostsim build of the same code.

Frames are 40x30, 4 bounces, N <= 6 (progress_cases' sizes); the display-only cases run on synthetic
buffers. Shared by tests/test_display.py (hostsim) and tests/test_display_gpu.py (gfx950).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import progress_cases as pc
import session_cases as sc
from progress_cases import H, N, NB, W
from session_cases import Session, assert_bits

from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_STATE, RT_OK, DisplayParams

EXPOSURES = (0.25, 1.5, 4.0)
GAMMAS = (1.0, 2.2, 2.4)
SHAPES = ((1, 1), (1, 8), (127, 5), (64, 4), (65, 3), (40, 30), (300, 7))  # (w, h)
# Case 5's bound on |hostsim - float64 model| over rgb: 4 x the largest difference measured over
# EXPOSURES x GAMMAS on model_buffer() (1.9404047e-07, at exposure 0.25 and gamma 2.4: DESIGN.md §11).
MODEL_MAX_MEASURED = 1.9404047e-07
MODEL_TOL = 4 * MODEL_MAX_MEASURED


# ------------------------------------------------------------------ the calls
def render_linear(s: Session, w=W, h=H, spp=N, nb=NB, fb=None) -> np.ndarray:
    fb = Session.blank(w, h) if fb is None else np.ascontiguousarray(fb, np.float32).copy()
    s.ok(s.L.rt_render_linear(s.ctx, w, h, spp, nb, _capi.ptr(fb)), "rt_render_linear")
    return fb


def render_linear_device(s: Session, shard, off, stride, w=W, h=H, spp=N, nb=NB) -> np.ndarray:
    d = s.array(np.ascontiguousarray(shard, np.float32))
    s.ok(s.L.rt_render_linear_device(s.ctx, w, h, spp, nb, sc._vp(d.ptr), off, stride, None), "rt_render_linear_device")
    return d.get()


def resolve_linear(s: Session, device: bool = False) -> np.ndarray:
    i = pc.info(s)
    shape = (i[7], i[0], 4)
    if device:
        d = s.array(np.full(shape, -3.0, np.float32))
        s.ok(s.L.rt_progress_resolve_linear_device(s.ctx, sc._vp(d.ptr), None), "rt_progress_resolve_linear_device")
        return d.get()
    out = np.full(shape, -3.0, np.float32)
    s.ok(s.L.rt_progress_resolve_linear(s.ctx, _capi.ptr(out)), "rt_progress_resolve_linear")
    return out


def display(s: Session, linear, exposure=1.5, gamma=2.2, flip=False, want=("rgba", "rgba8"), inplace=False,
            device=False, defaults=False):
    """(rgba or None, rgba8 or None) of rt_display / rt_display_device. inplace: rgba_out is the input
    buffer. defaults: params NULL. The outputs start from a pattern no result has."""
    lin = np.ascontiguousarray(linear, np.float32).copy()
    h, w = lin.shape[:2]
    p = None if defaults else ctypes.byref(DisplayParams(exposure, gamma, int(flip)))
    f_out, b_out = "rgba" in want, "rgba8" in want
    if device:
        d_in = s.array(lin)
        d_out = (d_in if inplace else s.array(np.full_like(lin, -5.0))) if f_out else None
        d_8 = s.array(np.full((h, w, 4), 77, np.uint8)) if b_out else None
        s.ok(s.L.rt_display_device(s.ctx, w, h, sc._vp(d_in.ptr), p, sc._vp(d_out.ptr) if d_out else None,
                                   sc._vp(d_8.ptr) if d_8 else None, None), "rt_display_device")
        return (d_out.get() if d_out else None, d_8.get() if d_8 else None)
    out = (lin if inplace else np.full_like(lin, -5.0)) if f_out else None
    out8 = np.full((h, w, 4), 77, np.uint8) if b_out else None
    s.ok(s.L.rt_display(s.ctx, w, h, _capi.ptr(lin), p, _capi.ptr(out), _capi.ptr(out8)), "rt_display")
    return out, out8


def rgba8_of(s: Session, rgba) -> np.ndarray:
    rgba = np.ascontiguousarray(rgba, np.float32)
    out = np.empty(rgba.shape, np.uint8)
    assert s.L.rt_image_to_rgba8(_capi.ptr(rgba), rgba.shape[0] * rgba.shape[1], _capi.ptr(out)) == RT_OK
    return out


def unbound(hostsim: bool) -> Session:
    """A context with nothing bound: the display stage needs no scene."""
    return Session(hostsim, name="display-unbound")


# ------------------------------------------------------------------ synthetic buffers
def model_buffer() -> np.ndarray:
    """48 x 20: rgb uniform in [0, 16], every 7th pixel's rgb exactly 0, column 5 denormal; the alpha
    cycles through 0, 0.25 and 1."""
    rng = np.random.default_rng(1105)
    a = (rng.random((20, 48, 4)) * 16.0).astype(np.float32)
    a.reshape(-1, 4)[::7, :3] = 0.0
    a[:, 5, :3] = (rng.integers(1, 1 << 23, (20, 3)).astype(np.uint32)).view(np.float32)
    a[..., 3] = np.asarray([0.0, 0.25, 1.0], np.float32)[np.arange(48) % 3]
    return a


def edge_buffer() -> np.ndarray:
    """16 x 3: every rgb edge value against every alpha of (0, 0.25, 1)."""
    inf = np.float32(np.inf)
    vals = np.asarray([np.nan, inf, -inf, -1.0, -0.0, 0.0, -1e-3, -16.0, 1.0, 1e-40, -1e-40, 3e38, -3e38, 88.0, 0.5, 2.0],
                      np.float32)
    a = np.empty((3, 16, 4), np.float32)
    a[..., 0] = vals
    a[..., 1] = vals[::-1]
    a[..., 2] = np.roll(vals, 5)
    a[..., 3] = np.asarray([0.0, 0.25, 1.0], np.float32)[:, None]
    return a


def shape_buffer(w: int, h: int) -> np.ndarray:
    """Values that spread over the 8-bit range after the tone-map, alpha included."""
    rng = np.random.default_rng([77, w, h])
    a = (rng.random((h, w, 4)) * 3.0).astype(np.float32)
    a[..., 3] = rng.random((h, w), dtype=np.float32) * np.float32(-0.6)  # (alpha out = 1 + 1.5 a: 0.1 .. 1)
    return a


def model(lin, exposure, gamma) -> np.ndarray:
    """rgb: (1 - exp(-x e)) ^ (1 / g) in float64."""
    x = lin[..., :3].astype(np.float64)
    return (1.0 - np.exp(-x * np.float64(np.float32(exposure)))) ** (1.0 / np.float64(np.float32(gamma)))


def model_alpha(lin, exposure) -> np.ndarray:
    """The alpha line in numpy float32: a = v[3] + 0; 1 + (-((-a) * e))."""
    a = lin[..., 3] + np.float32(0.0)
    return np.float32(1.0) + (-((-a) * np.float32(exposure)))


# ------------------------------------------------------------------ the cases
def case_round_trip(hostsim: bool, scene: str, base: str):
    """1: rt_display(rt_render_linear(fb0), defaults) is rt_render(fb0) and the oracle's frame; also in
    place, through the device forms, and with params NULL."""
    s = pc.session(hostsim, scene)
    fb0 = pc.base_of(base)
    lin = render_linear(s, fb=fb0)
    assert_bits(lin[..., 3], fb0[..., 3], s.where("rt_render_linear leaves the alpha"))
    want = s.render(W, H, N, NB, fb0)
    got, _ = display(s, lin)
    assert_bits(got, want, s.where(f"{scene} {base}: display(render_linear) vs rt_render"))
    assert_bits(got, pc.oracle_frame(s, scene, N, base), s.where(f"{scene} {base}: display(render_linear) vs the oracle"))
    assert_bits(display(s, lin, inplace=True, want=("rgba",))[0], want, s.where("in place"))
    assert_bits(display(s, lin, defaults=True, want=("rgba",))[0], want, s.where("params NULL"))
    assert_bits(display(s, lin, device=True)[0], want, s.where("rt_display_device"))
    assert_bits(display(s, lin, device=True, inplace=True, want=("rgba",))[0], want, s.where("rt_display_device in place"))
    s.close()


def checkpoint_arrays(s: Session):
    """(base, state, done) of the running progression, from rt_progress_save."""
    blob = pc.save(s)
    i = pc.info(s)
    n = i[7] * i[0] * 4
    body = np.frombuffer(blob[pc.HEADER:], np.float32)
    return body[:n].reshape(i[7], i[0], 4), body[n:].reshape(i[7], i[0], 4), i[3]


def numpy_linear(base, state, done) -> np.ndarray:
    out = base.copy()
    out[..., :3] = base[..., :3] + state[..., :3] / np.float32(done)
    return out


def case_linear_pinned(hostsim: bool, scene: str = "cornell"):
    """2: rt_progress_resolve_linear is numpy float32 base.rgb + state.rgb / done with the base's alpha, at
    done = 2 and 6; at done = N it is rt_render_linear into that base; device form = host form; the
    resolve changes no state."""
    s = pc.session(hostsim, scene)
    base0 = pc.base_of("random")
    pc.begin(s, base=base0)
    pc.advance(s, 2)
    for done in (2, N):
        if done == N:
            pc.advance(s, N - 2)
        base, state, d = checkpoint_arrays(s)
        assert d == done
        assert_bits(base, base0, s.where("the checkpoint's base"))
        got = resolve_linear(s)
        assert_bits(got, numpy_linear(base, state, done), s.where(f"resolve_linear at {done} vs numpy float32"))
        assert_bits(resolve_linear(s, device=True), got, s.where(f"resolve_linear_device at {done} vs the host form"))
        assert pc.save(s)[pc.HEADER:] == np.concatenate([base.ravel(), state.ravel()]).tobytes(), \
            s.where("a linear resolve changed the state")
    assert_bits(got, render_linear(s, fb=base0), s.where("resolve_linear at N vs rt_render_linear"))
    # the tone-mapped resolve after all those linear ones is still the frame
    assert_bits(pc.resolve(s), pc.oracle_frame(s, scene, N, "random"), s.where("rt_progress_resolve afterwards vs the oracle"))
    s.close()


def case_resolve_pure(hostsim: bool):
    """2: linear resolves between passes: a later advance ends at the same frame."""
    s = pc.session(hostsim, "cornell")
    pc.begin(s)
    pc.advance(s, 3)
    a, b = resolve_linear(s), resolve_linear(s, device=True)
    assert_bits(a, b, s.where("two linear resolves between passes"))
    pc.advance(s, 3)
    lin = resolve_linear(s)
    assert_bits(display(s, lin, want=("rgba",))[0], pc.oracle_frame(s, "cornell", N), s.where("display(resolve_linear) vs the oracle"))
    s.close()


def case_split(hostsim: bool, scene: str = "cornell"):
    """3: rt_progress_resolve_linear after [6], [1] * 6 and [3, 1, 2]: identical words."""
    s = pc.session(hostsim, scene)
    frames = []
    for split in ([6], [1] * 6, [3, 1, 2]):
        pc.begin(s, total=N)
        for k in split:
            pc.advance(s, k)
        frames.append(resolve_linear(s))
    assert_bits(frames[1], frames[0], s.where("[1] * 6 vs [6]"))
    assert_bits(frames[2], frames[0], s.where("[3, 1, 2] vs [6]"))
    assert_bits(frames[0], render_linear(s), s.where("[6] vs rt_render_linear"))
    s.close()


def case_shard(hostsim: bool):
    """4: rt_render_linear_device with row_offset 1, row_stride 3 is those rows of the whole linear frame."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    whole = render_linear(s, fb=base)
    assert_bits(render_linear_device(s, base[1::3], 1, 3), whole[1::3], s.where("rows 1::3 vs the whole linear frame"))
    assert_bits(render_linear_device(s, base, 0, 1), whole, s.where("the device form, whole frame"))
    s.close()


def case_multi(hostsim: bool):
    """4: a 2-shard context (hostsim: two host "devices"; gfx950: rt_create_multi_loopback over GPU 0
    twice) gives the single-device linear frame, and its display runs on the root device."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    want = render_linear(s, fb=base)
    s.close()
    m = Session(hostsim, name="display-multi", devices=[0, 1] if hostsim else [0, 0], loopback=not hostsim)
    pc.bind(m, "cornell")
    got = render_linear(m, fb=base)
    assert_bits(got, want, m.where("2 shards vs one device, linear"))
    assert_bits(render_linear_device(m, base[1::3], 1, 3), want[1::3], m.where("2 shards, rows 1::3"))
    assert_bits(display(m, got, want=("rgba",))[0], pc.oracle_frame(m, "cornell", N, "random"),
                m.where("display on a multi-device context vs the oracle"))
    m.close()


def case_model(hostsim: bool, exposure: float, gamma: float):
    """5: hostsim against the float64 model within MODEL_TOL (rgb) and numpy float32 (alpha); gfx950
    against hostsim, bit for bit."""
    lin = model_buffer()
    h = unbound(True)
    ref, ref8 = display(h, lin, exposure, gamma)
    if hostsim:
        d = np.abs(ref[..., :3].astype(np.float64) - model(lin, exposure, gamma))
        print(f"display model e={exposure} g={gamma}: max |hostsim - float64| = {d.max():.7e}")
        assert np.isfinite(ref).all()
        assert d.max() <= MODEL_TOL, f"exposure {exposure} gamma {gamma}: {d.max()} > {MODEL_TOL}"
        assert_bits(ref[..., 3], model_alpha(lin, exposure), "alpha vs numpy float32")
        assert (ref[..., :3][lin[..., :3] == 0] == 0).all(), "zero radiance displays as zero"
    else:
        s = unbound(False)
        for dev in (False, True):
            got, got8 = display(s, lin, exposure, gamma, device=dev)
            assert_bits(got, ref, f"gfx950 vs hostsim, e={exposure} g={gamma} device={dev}")
            assert np.array_equal(got8, ref8), f"gfx950 vs hostsim 8-bit, e={exposure} g={gamma} device={dev}"
        s.close()
    h.close()


def case_edges(hostsim: bool):
    """6: NaN, +-inf, negative radiance, -0.0 and the alphas 0, 0.25, 1: the 8-bit words are
    rt_image_to_rgba8 of the float output; gfx950 equals hostsim bit for bit."""
    lin = edge_buffer()
    h = unbound(True)
    for e, g in ((1.5, 2.2), (0.25, 1.0), (4.0, 2.4)):
        ref, ref8 = display(h, lin, e, g)
        assert np.array_equal(ref8, rgba8_of(h, ref)), f"hostsim 8-bit vs rt_image_to_rgba8, e={e} g={g}"
        if hostsim:
            r = ref[0, :, 0]  # (the values of edge_buffer in order)
            assert np.isnan(r[0]) and r[1] == 1.0 and r[4] == 0.0 and r[5] == 0.0, "NaN, +inf, -0.0, 0.0"
            assert np.isposinf(r[2]) if g != 1.0 else np.isneginf(r[2]), "-inf: powf(-inf, y)"
            assert (np.isnan(r[3]) and np.isnan(r[7])) if g != 1.0 else (r[3] < 0 and r[7] < 0), "powf of a negative"
            assert_bits(ref[..., 3], model_alpha(lin, e), "alpha vs numpy float32")
        else:
            s = unbound(False)
            for dev in (False, True):
                got, got8 = display(s, lin, e, g, device=dev)
                assert_bits(got, ref, f"edges: gfx950 vs hostsim, e={e} g={g} device={dev}")
                assert np.array_equal(got8, ref8), f"edges: 8-bit gfx950 vs hostsim, e={e} g={g} device={dev}"
                assert np.array_equal(got8, rgba8_of(s, got)), "edges: 8-bit vs rt_image_to_rgba8 of the float output"
            s.close()
    h.close()


def case_shape(hostsim: bool, w: int, h: int):
    """7: rgba8_out is rt_image_to_rgba8(rgba_out), rows reversed with flip_y; float only, 8-bit only and
    both agree; gfx950 (host and device forms) equals hostsim."""
    lin = shape_buffer(w, h)
    hs = unbound(True)
    ref, ref8 = display(hs, lin)
    assert np.array_equal(ref8, rgba8_of(hs, ref))
    assert len(np.unique(ref8)) > 1 or w * h == 1
    s = hs if hostsim else unbound(False)
    for dev in (False, True):
        both, both8 = display(s, lin, device=dev)
        assert_bits(both, ref, f"{w}x{h} device={dev}: float output")
        assert np.array_equal(both8, ref8), f"{w}x{h} device={dev}: 8-bit output"
        only, none8 = display(s, lin, want=("rgba",), device=dev)
        assert none8 is None
        assert_bits(only, both, f"{w}x{h} device={dev}: float only vs both")
        none, only8 = display(s, lin, want=("rgba8",), device=dev)
        assert none is None and np.array_equal(only8, both8), f"{w}x{h} device={dev}: 8-bit only vs both"
        fl, fl8 = display(s, lin, flip=True, device=dev)
        assert_bits(fl, both, f"{w}x{h} device={dev}: flip_y leaves the float output alone")
        assert np.array_equal(fl8, both8[::-1]), f"{w}x{h} device={dev}: flip_y reverses the 8-bit rows"
        assert np.array_equal(display(s, lin, flip=True, want=("rgba8",), device=dev)[1], both8[::-1])
    if not hostsim:
        s.close()
    hs.close()


def case_errors(hostsim: bool):
    """9: every RT_ERR_ARG and RT_ERR_STATE of the new calls."""
    s = unbound(hostsim)
    lin = shape_buffer(8, 4)
    out, out8 = np.empty_like(lin), np.empty((4, 8, 4), np.uint8)

    def rc(w=8, h=4, src=lin, p=None, o=out, o8=out8, device=False):
        pp = None if p is None else ctypes.byref(DisplayParams(*p))
        if device:  # (refused before any pointer is used: host pointers will do)
            return s.L.rt_display_device(s.ctx, w, h, _capi.ptr(src), pp, _capi.ptr(o), _capi.ptr(o8), None)
        return s.L.rt_display(s.ctx, w, h, _capi.ptr(src), pp, _capi.ptr(o), _capi.ptr(o8))

    inf, nan = float("inf"), float("nan")
    for device in (False, True):
        for what, kw in (("width 0", dict(w=0)), ("height -1", dict(h=-1)), ("input NULL", dict(src=None)),
                         ("exposure inf", dict(p=(inf, 2.2, 0))), ("exposure NaN", dict(p=(nan, 2.2, 0))),
                         ("gamma 0", dict(p=(1.5, 0.0, 0))), ("gamma < 0", dict(p=(1.5, -2.2, 0))),
                         ("gamma inf", dict(p=(1.5, inf, 0))), ("gamma NaN", dict(p=(1.5, nan, 0))),
                         ("both outputs NULL", dict(o=None, o8=None)), ("2^27 pixels", dict(w=1 << 14, h=1 << 13)),
                         ("rgba8_out is the input", dict(o8=lin)), ("rgba8_out inside the input", dict(o8=lin[2:])),
                         ("rgba8_out is rgba_out", dict(o8=out)), ("rgba8_out inside rgba_out", dict(o8=out[3:])),
                         ("rgba_out overlaps the input without being it", dict(o=lin[1:]))):
            assert rc(device=device, **kw) == RT_ERR_ARG and s.error(), s.where(f"rt_display device={device}: {what}")
    # alignment: the device form wants 16 bytes for the float frames and 4 for the bytes; the host form takes any
    off_f = np.zeros(lin.size + 4, np.float32)[1:1 + lin.size].reshape(lin.shape)
    off_o = np.zeros(lin.size + 4, np.float32)[1:1 + lin.size].reshape(lin.shape)
    off_8 = np.zeros(out8.size + 4, np.uint8)[1:1 + out8.size].reshape(out8.shape)
    assert off_f.ctypes.data % 16 == 4 and off_8.ctypes.data % 4 == 1
    off_f[...] = lin
    for what, kw in (("input off by 4 bytes", dict(src=off_f)), ("rgba_out off by 4 bytes", dict(o=off_o)),
                     ("rgba8_out off by 1 byte", dict(o8=off_8))):
        assert rc(device=True, **kw) == RT_ERR_ARG and "aligned" in s.error(), s.where(f"rt_display_device: {what}")
    assert rc(src=off_f, o=off_o, o8=off_8) == RT_OK, s.where(f"the host form with unaligned buffers: {s.error()}")
    assert rc() == RT_OK
    assert_bits(off_o, out, s.where("unaligned host buffers: the float output"))
    assert np.array_equal(off_8, out8), s.where("unaligned host buffers: the 8-bit output")
    assert s.L.rt_display(None, 8, 4, _capi.ptr(lin), None, _capi.ptr(out), None) == RT_ERR_ARG, "ctx NULL"
    assert rc(p=(-1.5, 2.2, 1)) == RT_OK, s.where(f"a negative exposure is finite: {s.error()}")
    # the linear renders report what rt_render reports
    fb = Session.blank(8, 4)
    assert s.L.rt_render_linear(s.ctx, 8, 4, 1, 1, _capi.ptr(fb)) == RT_ERR_STATE and s.error(), "no scene"
    assert s.L.rt_render_linear_device(s.ctx, 8, 4, 1, 1, _capi.ptr(fb), 0, 1, None) == RT_ERR_STATE, "no scene (device)"
    assert s.L.rt_progress_resolve_linear(s.ctx, _capi.ptr(fb)) == RT_ERR_STATE, "no progression"
    assert s.L.rt_progress_resolve_linear_device(s.ctx, _capi.ptr(fb), None) == RT_ERR_STATE, "no progression (device)"
    s.set_named_scene("cornell")
    assert s.L.rt_render_linear(s.ctx, 8, 4, 1, 1, _capi.ptr(fb)) == RT_ERR_STATE, "no BVH"
    s.build_bvh()
    assert s.L.rt_render_linear(s.ctx, 8, 4, 1, 1, _capi.ptr(fb)) == RT_ERR_STATE and "environment" in s.error(), "no env"
    s.set_env(sc.rt_cases.sky("S"))
    assert s.L.rt_render_linear(s.ctx, 8, 4, 1, 1, _capi.ptr(fb)) == RT_ERR_STATE and "camera" in s.error(), "no camera"
    s.set_camera(sc.camera_of("cornell"))
    for what, args in (("width 0", (0, 4, 1, 1)), ("samples 0", (8, 4, 0, 1)), ("bounces -1", (8, 4, 1, -1))):
        assert s.L.rt_render_linear(s.ctx, *args, _capi.ptr(fb)) == RT_ERR_ARG, s.where(f"rt_render_linear: {what}")
    assert s.L.rt_render_linear(s.ctx, 8, 4, 1, 1, None) == RT_ERR_ARG, "fb NULL"
    for what, (off, stride) in (("stride 0", (0, 0)), ("offset < 0", (-1, 2)), ("offset >= stride", (2, 2))):
        assert s.L.rt_render_linear_device(s.ctx, 8, 4, 1, 1, _capi.ptr(fb), off, stride, None) == RT_ERR_ARG, what
    assert s.L.rt_render_linear_device(s.ctx, 8, 4, 1, 1, None, 0, 1, None) == RT_ERR_ARG, "d_fb NULL"
    pc.begin(s, total=2, w=8, h=4)
    assert s.L.rt_progress_resolve_linear(s.ctx, _capi.ptr(fb)) == RT_ERR_STATE and s.error(), "done == 0"
    assert s.L.rt_progress_resolve_linear_device(s.ctx, _capi.ptr(fb), None) == RT_ERR_STATE, "done == 0 (device)"
    pc.advance(s, 1)
    assert s.L.rt_progress_resolve_linear(s.ctx, None) == RT_ERR_ARG, "resolve into NULL"
    s.set_camera(s.cam)  # (a rebind ends the progression)
    assert s.L.rt_progress_resolve_linear(s.ctx, _capi.ptr(fb)) == RT_ERR_STATE, "after a rebind"
    s.close()


def case_python(hostsim: bool):
    """10: RenderKernel.render_linear, display and progress_resolve_linear agree with the C calls."""
    import rt_amd
    from conftest import parsed_scene
    P = parsed_scene("cornell")
    base = pc.base_of("random")

    def kernel(img):
        rk = rt_amd.RenderKernel(W, H, N, NB, img, P.triangles, P.materials, P.emissive_triangle_indices,
                                 P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sc.rt_cases.sky("S")),
                                 None, device=0, hostsim=hostsim)
        cam = sc.camera_of("cornell")
        rk.set_camera(rt_amd.Camera(cam[:16].reshape(4, 4), float(cam[16])))
        return rk

    s = pc.session(hostsim, "cornell")
    lin_c = render_linear(s, fb=base)
    img = rt_amd.Image(W, H, pixels=base.copy())
    rk = kernel(img)
    rk.render_linear()
    assert_bits(img.pixels, lin_c, "RenderKernel.render_linear vs rt_render_linear")
    shown = rk.display()
    assert isinstance(shown, rt_amd.Image)
    assert_bits(shown.pixels, s.render(W, H, N, NB, base), "RenderKernel.display(render_linear) vs rt_render")
    assert_bits(img.pixels, lin_c, "display() left the linear frame alone")
    for e, g, flip in ((0.5, 2.4, True), (4.0, 1.0, False)):
        want, want8 = display(s, lin_c, e, g, flip)
        got, got8 = rk.display(img, exposure=e, gamma=g, flip_y=flip, want=("rgba", "rgba8"))
        assert_bits(got.pixels, want, f"RenderKernel.display e={e} g={g}")
        assert np.array_equal(got8, want8) and got8.dtype == np.uint8
        assert np.array_equal(rk.display(img, e, g, flip, want="rgba8"), want8)
        got8b, gotb = rk.display(img, e, g, flip, want=("rgba8", "rgba"))
        assert np.array_equal(got8b, want8) and np.array_equal(gotb.pixels.view(np.uint32), got.pixels.view(np.uint32))
    prog = rt_amd.Image(W, H, pixels=base.copy())
    rp = kernel(prog)
    rp.progress_begin()
    rp.progress_advance(2)
    pc.begin(s, base=base)
    pc.advance(s, 2)
    out = rt_amd.Image(W, H)
    assert rp.progress_resolve_linear(out) is out
    assert_bits(out.pixels, resolve_linear(s), "RenderKernel.progress_resolve_linear vs the C call at 2 of 6")
    rp.progress_advance(4)
    assert_bits(rp.progress_resolve_linear().pixels, lin_c, "progress_resolve_linear at N vs rt_render_linear")
    rp.progress_end()
    s.close()
