"""Progressive rendering (rt_progress_*, include/rt_hip.h): a frame of N samples rendered in passes
on one context, held bitwise to rt_render of the same context and to the oracle, however the total
is split, under every wave plan, through interleaved calls, a checkpoint and the rebinds that end it.

Frames are 40x30, 4 bounces, N <= 6: the pause logic does not depend on frame size. Shared by
tests/test_progress.py (hostsim) and tests/test_progress_gpu.py (gfx950), as session_cases.py is.

Helpers only: no tests here."""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import rt_cases
import session_cases as sc
from conftest import parsed_scene
from session_cases import Session, assert_bits

from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_STATE, RT_OK

W, H, NB, N = 40, 30, 4, 6
SCENES = ("cornell", "fan", "sphere", "brute")
SPLITS = ([6], [1] * 6, [3, 1, 2], [5, 1])
# the wave plans of case 3 (rt_test_schedule): the sessions' three, then the ones the issue names
SCHEDULES = dict(sc.SCHEDULES, spec_cam0=dict(spec_cam=0), spec_cam1=dict(spec_cam=1), spec_cam2=dict(spec_cam=2),
                 tail1=dict(tail_paths=1, tail_enter=1000), fast_lane=dict(fast_k=64, fast_spp=0.0))
HEADER = 40  # bytes: magic, version, the eight info words

# the oracle's frames by (scene, spp, base, shard): computed once, read-only
_want: dict = {}


def bind(s: Session, scene: str):
    if scene == "sphere":
        P = parsed_scene("cornell12")
        mats, mi, sph = rt_cases.sphere_buffers(dict(spheres=sc._sphere_entry()), P, P.materials)
        s.set_scene(P.triangles, mi, mats, P.emissive_triangle_indices, sph)
        cam = sc.camera_of("cornell12")
    elif scene == "brute":
        s.set_named_scene("cornell12")
        cam = sc.camera_of("cornell12")
    else:
        s.set_named_scene(scene)
        cam = sc.camera_of(scene)
    s.build_bvh()
    s.set_env(rt_cases.sky("S"))
    s.set_camera(cam)
    if scene == "brute":
        s.set_intersect_mode(False)


def session(hostsim: bool, scene: str = "cornell", schedule=None) -> Session:
    s = Session(hostsim, name=f"progress-{scene}", schedule=schedule)
    bind(s, scene)
    return s


def base_of(kind: str) -> np.ndarray:
    """'blank': (0, 0, 0, 1) per pixel; 'random': values in [0, 1) and alpha 0.25."""
    fb = Session.blank(W, H)
    if kind == "random":
        fb[..., :3] = np.random.default_rng(4711).random((H, W, 3), dtype=np.float32)
        fb[..., 3] = 0.25
    return fb


def oracle_frame(s: Session, scene: str, spp: int, base: str = "blank", nb: int = NB) -> np.ndarray:
    key = (scene, spp, base, nb)
    if key not in _want:
        fb = s.oracle().render(s.cam, W, H, spp, nb, fb=base_of(base).copy())[0]
        fb.setflags(write=False)
        _want[key] = fb
    return _want[key]


# ------------------------------------------------------------------ the calls
def begin_rc(s, total=N, nb=NB, base=None, off=0, stride=1, w=W, h=H):
    b = None if base is None else np.ascontiguousarray(base[off::stride], np.float32)
    return s.L.rt_progress_begin(s.ctx, w, h, total, nb, _capi.ptr(b), off, stride)


def begin(s, **kw):
    s.ok(begin_rc(s, **kw), "rt_progress_begin")


def advance_rc(s, k):
    return s.L.rt_progress_advance(s.ctx, k, None)


def advance(s, k):
    s.ok(advance_rc(s, k), f"rt_progress_advance({k})")


def info(s) -> list:
    out = np.zeros(8, np.int32)
    s.ok(s.L.rt_progress_info(s.ctx, _capi.ptr(out)), "rt_progress_info")
    return [int(v) for v in out]


def resolve(s, device: bool = False) -> np.ndarray:
    """The shard's rows [rows_local, W, 4]; device: through rt_progress_resolve_device."""
    i = info(s)
    shape = (i[7], i[0], 4)
    if device:
        d = s.array(np.full(shape, -3.0, np.float32))
        s.ok(s.L.rt_progress_resolve_device(s.ctx, sc._vp(d.ptr), None), "rt_progress_resolve_device")
        return d.get()
    out = np.full(shape, -3.0, np.float32)
    s.ok(s.L.rt_progress_resolve(s.ctx, _capi.ptr(out)), "rt_progress_resolve")
    return out


def save(s) -> bytes:
    n = s.L.rt_progress_save(s.ctx, None, 0)
    assert n > 0, s.where(f"rt_progress_save(NULL, 0) = {n}: {s.error()}")
    buf = ctypes.create_string_buffer(n)
    assert s.L.rt_progress_save(s.ctx, buf, n) == n, s.where(f"rt_progress_save: {s.error()}")
    return buf.raw


def load_rc(s, data: bytes):
    return s.L.rt_progress_load(s.ctx, ctypes.create_string_buffer(data, len(data)), len(data))


def run_split(s, split, resolves: bool = False, **kw) -> np.ndarray:
    begin(s, total=sum(split), **kw)
    for k in split:
        advance(s, k)
        if resolves:
            resolve(s)
    return resolve(s)


# ------------------------------------------------------------------ the cases
def case_split(hostsim: bool, scene: str, split, base: str = "blank"):
    """1: the resolve after the last pass is rt_render of the same context and the oracle's frame."""
    s = session(hostsim, scene)
    got = run_split(s, split, base=base_of(base))
    assert info(s)[2:4] == [N, N], s.where(f"info after {split}")
    assert_bits(got, s.render(W, H, N, NB, base_of(base)), s.where(f"{scene} split {split} vs rt_render"))
    assert_bits(got, oracle_frame(s, scene, N, base), s.where(f"{scene} split {split} vs the oracle"))
    assert_bits(resolve(s, device=True), got, s.where("rt_progress_resolve_device vs rt_progress_resolve"))
    s.close()


def case_shard(hostsim: bool):
    """1: rows 1, 4, 7, ... of the frame, non-trivial base: the seed uses the true y."""
    s = session(hostsim, "cornell")
    base = base_of("random")
    got = run_split(s, [3, 1, 2], base=base, off=1, stride=3)
    assert info(s) == [W, H, N, N, NB, 1, 3, (H - 1 + 2) // 3], s.where("info of the shard")
    assert_bits(got, s.render_device(W, H, N, NB, base[1::3], 1, 3), s.where("shard vs rt_render_device"))
    assert_bits(got, oracle_frame(s, "cornell", N, "random")[1::3], s.where("shard vs the oracle's rows"))
    s.close()


def case_seed31(hostsim: bool, scene: str = "cornell"):
    """2: where x*y == 0 the seed is 31 whatever the count, so the intermediate resolve's row 0 and
    column 0 are the oracle's s-sample frame there. Whole frame: the GPU against the hostsim build."""
    s = session(hostsim, scene)
    h = None if hostsim else session(True, scene)
    begin(s)
    if h:
        begin(h)
    done = 0
    for k, want_done in ((1, 1), (1, 2), (3, 5)):
        advance(s, k)
        done += k
        assert done == want_done and info(s)[3] == done
        got = resolve(s)
        want = oracle_frame(s, scene, done)
        assert_bits(got[0], want[0], s.where(f"row 0 after {done} of {N} vs the oracle's {done}-sample frame"))
        assert_bits(got[:, 0], want[:, 0], s.where(f"column 0 after {done} of {N} vs the oracle's {done}-sample frame"))
        if h:
            advance(h, k)
            assert_bits(got, resolve(h), s.where(f"whole frame after {done} of {N} vs the hostsim build"))
    s.close()
    if h:
        h.close()


def case_schedule(hostsim: bool, name: str):
    """3: the [3, 1, 2] split under one wave plan."""
    s = session(hostsim, "cornell", schedule=SCHEDULES[name])
    got = run_split(s, [3, 1, 2])
    assert_bits(got, oracle_frame(s, "cornell", N), s.where(f"schedule {name} vs the oracle"))
    s.close()


def case_schedule_change(hostsim: bool):
    """3: every pass under another plan (lanes, tail, fast lane): the state is indexed like the framebuffer."""
    s = session(hostsim, "cornell")
    begin(s)
    for k, plan in zip([3, 1, 2], (dict(lanes=1, tail_paths=0), dict(lanes=3, tail_paths=1, tail_enter=1000),
                                   dict(lanes=2, fast_k=64, fast_spp=0.0, spec_cam=2))):
        s.schedule("reset")
        for key, v in plan.items():
            s.schedule(key, v)
        advance(s, k)
    assert_bits(resolve(s), oracle_frame(s, "cornell", N), s.where("a plan per pass vs the oracle"))
    s.close()


def last_iterations(s) -> int:
    return -1 if s.hostsim else int(s.L.rt_device_last_iterations(s.ctx))


def case_edges(hostsim: bool):
    """4: bounces 0, N = 1, advance past the end, advance after completion."""
    s = session(hostsim, "cornell")
    got = run_split(s, [2, 1, 3], nb=0)
    assert_bits(got, oracle_frame(s, "cornell", N, nb=0), s.where("0 bounces vs the oracle"))
    got = run_split(s, [1])
    assert_bits(got, oracle_frame(s, "cornell", 1), s.where("N = 1 vs the oracle"))
    begin(s)
    advance(s, 4)
    advance(s, 100)
    assert info(s)[3] == N, s.where("advance(100) with 2 left")
    got = resolve(s)
    s.render(8, 8, 1, 1)  # (a short render: the iteration count below is its, until a pass runs)
    its = last_iterations(s)
    assert advance_rc(s, 1) == RT_OK and info(s)[3] == N, s.where("advance after completion")
    assert last_iterations(s) == its, s.where("advance after completion launched a pass")
    assert_bits(resolve(s), got, s.where("the result after the idle advance"))
    assert_bits(got, oracle_frame(s, "cornell", N), s.where("4 + 100 vs the oracle"))
    s.close()


def case_pure(hostsim: bool):
    """5: resolves change nothing."""
    s = session(hostsim, "cornell")
    begin(s)
    advance(s, 3)
    a, b = resolve(s), resolve(s, device=True)
    assert_bits(a, b, s.where("two resolves between passes"))
    advance(s, 1)
    resolve(s)
    advance(s, 2)
    assert_bits(resolve(s), oracle_frame(s, "cornell", N), s.where("with intermediate resolves vs the oracle"))
    s.close()


def case_interleave(hostsim: bool):
    """6: other calls on the context between passes leave the progression alone, and answer right."""
    s = session(hostsim, "cornell")
    begin(s)
    advance(s, 3)
    s.step = 1
    s.check_frame(24, 18, 2, 3, "another size")
    advance(s, 1)
    rays = s.rays()
    assert_bits(s.query(rays), sc.records(s.oracle(), rays), s.where("rt_query between passes vs the oracle"))
    alb, nd = s.check_features(W, H)
    preview = np.ascontiguousarray(resolve(s))
    den = s.denoise(preview, alb, nd, 2, 1.0)
    hs = s if hostsim else session(True, "cornell")
    assert_bits(den, hs.denoise(preview, alb, nd, 2, 1.0), s.where("rt_denoise of the preview vs the hostsim build"))
    advance(s, 2)
    assert_bits(resolve(s), oracle_frame(s, "cornell", N), s.where("interleaved vs the oracle"))
    s.close()


def case_checkpoint(hostsim: bool):
    """7: save at 2 of 6, a new context, load, advance 4; the round trip; the corrupt headers."""
    s = session(hostsim, "cornell")
    base = base_of("random")
    begin(s, base=base)
    advance(s, 2)
    blob = save(s)
    assert len(blob) == HEADER + 2 * 16 * W * H, "the checkpoint's size"
    assert struct.unpack("<8i", blob[8:HEADER]) == (W, H, N, 2, NB, 0, 1, H), "the header's info words"
    s.close()
    t = session(hostsim, "cornell")
    assert load_rc(t, blob) == RT_OK, t.where(f"rt_progress_load: {t.error()}")
    assert info(t) == [W, H, N, 2, NB, 0, 1, H]
    assert save(t) == blob, "save -> load -> save"
    advance(t, 4)
    assert_bits(resolve(t), oracle_frame(t, "cornell", N, "random"), t.where("resumed in a new context vs the oracle"))

    def header(**kw):
        words = list(struct.unpack("<10i", blob[:HEADER]))
        for k, v in kw.items():
            words[dict(magic=0, version=1, w=2, total=4, done=5)[k]] = v
        return struct.pack("<10i", *words) + blob[HEADER:]

    for what, bad in (("magic", header(magic=0x12345678)), ("version", header(version=99)), ("short", blob[:-16]),
                      ("long", blob + b"\0" * 16), ("width", header(w=W + 1)), ("done > total", header(done=N + 1)),
                      ("no header", blob[:12])):
        assert load_rc(t, bad) == RT_ERR_ARG and t.error(), t.where(f"corrupt checkpoint: {what}")
    assert info(t)[3] == N, t.where("a refused load left the progression alone")
    u = Session(hostsim, name="progress-unbound")
    assert load_rc(u, blob) == RT_ERR_STATE, "rt_progress_load without a scene"
    u.close()
    t.close()


def _rebinds(s: Session):
    P = parsed_scene("cornell")
    return {
        "rt_set_scene": lambda: (s.set_scene(P.triangles, P.material_indices, P.materials, P.emissive_triangle_indices),
                                 s.build_bvh()),
        "rt_build_bvh": lambda: s.build_bvh(16, 4),
        "rt_set_bvh_preorder": lambda: s.set_bvh_preorder(s.bvh_dump(), s.bvh),
        "rt_set_env": lambda: s.set_env(rt_cases.sky("S")),
        "rt_set_camera": lambda: s.set_camera(s.cam),
        "rt_set_materials": lambda: s.set_materials(s.mats),
        "rt_set_intersect_mode": lambda: s.set_intersect_mode(True),
    }


def case_invalidation(hostsim: bool):
    """8: every rebind ends the progression."""
    s = session(hostsim, "cornell")
    out = np.zeros((H, W, 4), np.float32)
    for name, call in _rebinds(s).items():
        begin(s)
        advance(s, 1)
        call()
        assert advance_rc(s, 1) == RT_ERR_STATE and s.error(), s.where(f"advance after {name}")
        assert s.L.rt_progress_resolve(s.ctx, _capi.ptr(out)) == RT_ERR_STATE, s.where(f"resolve after {name}")
        assert s.L.rt_progress_info(s.ctx, _capi.ptr(np.zeros(8, np.int32))) == RT_ERR_STATE
        assert s.L.rt_progress_save(s.ctx, None, 0) == RT_ERR_STATE, s.where(f"save after {name}")
    # a begin during a progression replaces it
    begin(s)
    advance(s, 5)
    assert_bits(run_split(s, [5, 1]), oracle_frame(s, "cornell", N), s.where("a second begin replaces the first"))
    s.L.rt_progress_end(s.ctx)
    s.L.rt_progress_end(s.ctx)
    assert advance_rc(s, 1) == RT_ERR_STATE, s.where("advance after rt_progress_end")
    s.close()


def case_errors(hostsim: bool):
    """8: the argument and state errors."""
    s = session(hostsim, "cornell")
    out = np.zeros((H, W, 4), np.float32)
    for what, kw in (("width 0", dict(w=0)), ("height -1", dict(h=-1)), ("total 0", dict(total=0)),
                     ("bounces -1", dict(nb=-1)), ("stride 0", dict(stride=0)), ("offset < 0", dict(off=-1)),
                     ("offset >= stride", dict(off=2, stride=2)), ("offset >= height", dict(off=H, stride=H + 5))):
        assert begin_rc(s, **kw) == RT_ERR_ARG and s.error(), s.where(f"rt_progress_begin: {what}")
    assert advance_rc(s, 1) == RT_ERR_STATE, s.where("advance without a progression")
    begin(s)
    assert s.L.rt_progress_resolve(s.ctx, _capi.ptr(out)) == RT_ERR_STATE, s.where("resolve with done == 0")
    for k in (0, -3):
        assert advance_rc(s, k) == RT_ERR_ARG, s.where(f"advance({k})")
    advance(s, 1)
    assert s.L.rt_progress_resolve(s.ctx, None) == RT_ERR_ARG, s.where("resolve into NULL")
    s.close()
    u = Session(hostsim, name="progress-unbound")
    assert begin_rc(u) == RT_ERR_STATE and u.error(), "rt_progress_begin without a scene"
    u.close()
    if hostsim:  # (a multi-device context of the hostsim build: the shards are host threads)
        m = Session(True, name="progress-multi", devices=[0, 1])
        bind(m, "cornell")
        assert begin_rc(m) == RT_ERR_ARG and "multi-device" in m.error(), "a multi-device context"
        m.close()


def case_python(hostsim: bool):
    """9: rt_amd.RenderKernel's progress_* methods, the [3, 1, 2] split with a checkpoint in it."""
    import rt_amd
    P = parsed_scene("cornell")
    base = base_of("random")

    def kernel(img):
        rk = rt_amd.RenderKernel(W, H, N, NB, img, P.triangles, P.materials, P.emissive_triangle_indices,
                                 P.material_indices, None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(rt_cases.sky("S")),
                                 None, device=0, hostsim=hostsim)
        cam = sc.camera_of("cornell")
        rk.set_camera(rt_amd.Camera(cam[:16].reshape(4, 4), float(cam[16])))
        return rk

    img = rt_amd.Image(W, H, pixels=base.copy())
    rk = kernel(img)
    rk.progress_begin()
    assert rk.progress_advance(3) == 3
    blob = rk.progress_save()
    rk2 = kernel(rt_amd.Image(W, H))
    rk2.progress_load(blob)
    assert rk2.progress_advance(1) == 4 and rk2.progress_advance(2) == 6
    assert rk2.progress_info()["total"] == N
    out = rk2.progress_resolve()
    ref = rt_amd.Image(W, H, pixels=base.copy())
    kernel(ref).render()
    assert_bits(out.pixels, ref.pixels, "RenderKernel.progress_* vs RenderKernel.render")
    rk2.progress_end()
