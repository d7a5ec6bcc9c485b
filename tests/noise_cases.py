"""The noise estimate of a tracked progression (rt_progress_noise_track, rt_progress_noise,
rt_progress_noise_device, checkpoint version 2; include/rt_hip.h). The reference is restate(): the
definition in numpy float32, written here and never calling the library. Injected states (packed as
version-2 checkpoints and loaded) pin the per-pixel arithmetic, the tile tree and the frame statistics;
renders pin the fold, that tracking changes no frame, the checkpoint and the row shard.

Frames are 40x30, 4 bounces, N <= 6 (progress_cases' sizes; 40x30 has partial tiles on both edges),
except case 7, which compares 4 samples with 64. Shared by tests/test_noise.py (hostsim) and
tests/test_noise_gpu.py (gfx950).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import display_cases as dc
import progress_cases as pc
import session_cases as sc
from progress_cases import H, N, NB, W
from session_cases import Session, assert_bits

from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_STATE, RT_OK, NoiseStats

SEED = 2207                      # of every injected buffer below
SHAPES = ((1, 1), (8, 8), (9, 1), (1, 9), (17, 9), (40, 30), (64, 8))  # (w, h)
HALVES = ((1, 1), (3, 3), (2, 4), (5, 1))                              # (nA, nB)
SPLITS = ([1] * 6, [3, 1, 2], [2, 4])
THRESHOLD = 0.05
MAGIC, HEADER2 = 0x47505452, pc.HEADER + 8
STAT_KEYS = ("tiles", "tiles_over", "nonfinite", "max_tile", "samples_a", "samples_b", "passes")
f32 = np.float32


# ------------------------------------------------------------------ the reference (numpy float32)
def restate(state, half, n_a: int, n_b: int, threshold: float, passes: int):
    """(pixel_err [rows, w], tile_err [th, tw], stats) of the definition. state, half: [rows, w, 4]."""
    state, half = np.asarray(state, f32), np.asarray(half, f32)
    rows, w = state.shape[:2]
    n_all, fa = f32(n_a + n_b), f32(n_a)
    with np.errstate(all="ignore"):
        k = np.sqrt(f32(n_a) / f32(n_b))
        m, a = state[..., :3] / n_all, half[..., :3] / fa
        d = (np.abs(m[..., 0] - a[..., 0]) + np.abs(m[..., 1] - a[..., 1])) + np.abs(m[..., 2] - a[..., 2])
        e = (k * d) / np.sqrt(f32(0.01) + ((m[..., 0] + m[..., 1]) + m[..., 2]))
    assert e.dtype == f32 and k.dtype == f32
    th, tw = (rows + 7) // 8, (w + 7) // 8
    fin = np.isfinite(e)
    pad = np.zeros((th * 8, tw * 8), f32)
    pad[:rows, :w] = np.where(fin, e, f32(0.0))
    v = pad.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th, tw, 64)  # element l: (l % 8, l / 8) of the tile
    with np.errstate(all="ignore"):
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
        count = np.minimum(8, w - 8 * np.arange(tw))[None, :] * np.minimum(8, rows - 8 * np.arange(th))[:, None]
        tile = v[..., 0] / count.astype(f32)
    assert tile.dtype == f32
    stats = dict(tiles=th * tw, tiles_over=int((tile > f32(threshold)).sum()), nonfinite=int((~fin).sum()),
                 max_tile=f32(tile.max()), samples_a=n_a, samples_b=n_b, passes=passes)
    return e, tile, stats


def numpy_fold(states):
    """half after the passes whose states (rgb sums saved after each pass, [rows, w, 4]) are given: around
    every even-numbered pass, half = half - state before it, then half = half + state after it."""
    half = np.zeros_like(states[0])
    prev = np.zeros_like(states[0])
    with np.errstate(all="ignore"):
        for p, st in enumerate(states):
            if p % 2 == 0:
                half[..., :3] = half[..., :3] - prev[..., :3]
                half[..., :3] = half[..., :3] + st[..., :3]
            prev = st
    return half


# ------------------------------------------------------------------ checkpoints
def pack_v2(base, state, half, total, done, passes, n_a, h=None, off=0, stride=1, nb=NB, version=2) -> bytes:
    rows, w = state.shape[:2]
    h = rows if h is None else h
    head = struct.pack("<10i", MAGIC, version, w, h, total, done, nb, off, stride, rows) + struct.pack("<2i", passes, n_a)
    return head + b"".join(np.ascontiguousarray(a, f32).tobytes() for a in (base, state, half))


def parse(blob: bytes) -> dict:
    hd = struct.unpack("<10i", blob[:pc.HEADER])
    w, rows, version = hd[2], hd[9], hd[1]
    out = dict(version=version, w=w, h=hd[3], total=hd[4], done=hd[5], rows=rows)
    at = pc.HEADER
    if version == 2:
        out["passes"], out["n_a"] = struct.unpack("<2i", blob[at:at + 8])
        at += 8
    body = np.frombuffer(blob[at:], f32)
    n = rows * w * 4
    assert body.size == (3 if version == 2 else 2) * n, "the checkpoint's size"
    for i, k in enumerate(("base", "state", "half")[:body.size // n]):
        out[k] = body[i * n:(i + 1) * n].reshape(rows, w, 4)
    return out


# ------------------------------------------------------------------ the calls
def track_rc(s):
    return s.L.rt_progress_noise_track(s.ctx)


def track(s):
    s.ok(track_rc(s), "rt_progress_noise_track")


def noise_rc(s, threshold=THRESHOLD, stats=True):
    st = NoiseStats()
    return s.L.rt_progress_noise(s.ctx, threshold, ctypes.byref(st) if stats else None, None, None)


def noise(s, threshold=THRESHOLD, device: bool = False, maps: bool = True):
    """(pixel_err, tile_err, stats dict) of rt_progress_noise, or of rt_progress_noise_device read back."""
    i = pc.info(s)
    rows, w = i[7], i[0]
    th, tw = (rows + 7) // 8, (w + 7) // 8
    if device:
        d_st = s.array(np.full(8, -9, np.int32))
        d_px = s.array(np.full((rows, w), -5.0, f32)) if maps else None
        d_tl = s.array(np.full((th, tw), -5.0, f32)) if maps else None
        s.ok(s.L.rt_progress_noise_device(s.ctx, threshold, sc._vp(d_st.ptr), sc._vp(d_px.ptr) if maps else None,
                                          sc._vp(d_tl.ptr) if maps else None, None), "rt_progress_noise_device")
        st = d_st.get()  # (the default stream: the download waits for the query)
        assert int(st[7]) == 0, s.where("the eighth stat word")
        stats = dict(tiles=int(st[0]), tiles_over=int(st[1]), nonfinite=int(st[2]), max_tile=st[3:4].view(f32)[0],
                     samples_a=int(st[4]), samples_b=int(st[5]), passes=int(st[6]))
        return (d_px.get() if maps else None, d_tl.get() if maps else None, stats)
    st = NoiseStats()
    px = np.full((rows, w), -5.0, f32) if maps else None
    tl = np.full((th, tw), -5.0, f32) if maps else None
    s.ok(s.L.rt_progress_noise(s.ctx, threshold, ctypes.byref(st), _capi.ptr(px), _capi.ptr(tl)), "rt_progress_noise")
    return px, tl, {k: (f32(st.max_tile) if k == "max_tile" else int(getattr(st, k))) for k in STAT_KEYS}


def assert_noise(got, want, msg):
    (px, tl, st), (wpx, wtl, wst) = got, want
    if px is not None:
        assert_bits(px, wpx, f"{msg}: pixel map")
        assert_bits(tl, wtl, f"{msg}: tile map")
    for k in STAT_KEYS:
        if k == "max_tile":
            assert f32(st[k]).view(np.uint32) == f32(wst[k]).view(np.uint32), f"{msg}: max_tile {st[k]!r} != {wst[k]!r}"
        else:
            assert st[k] == wst[k], f"{msg}: {k} {st[k]} != {wst[k]}"


# ------------------------------------------------------------------ injected states
EDGE_KINDS = ("zeros", "exact", "negative", "state_nan", "state_pinf", "state_ninf", "half_nan", "half_pinf", "half_ninf",
              "denormal", "huge", "ordinary", "ordinary")


def ordinary(w, h, n_a, n_b):
    """(base, state, half): positive sums; half near state * nA / N; the state's fourth word holds RNG bits."""
    rng = np.random.default_rng([SEED, w, h, n_a, n_b])
    n = n_a + n_b
    base = rng.random((h, w, 4), dtype=f32)
    state = np.empty((h, w, 4), f32)
    state[..., :3] = (rng.random((h, w, 3), dtype=f32) * f32(2.0) + f32(0.01)) * f32(n)
    state[..., 3] = rng.integers(1, 1 << 31, (h, w)).astype(np.uint32).view(f32)
    half = np.zeros((h, w, 4), f32)
    half[..., :3] = state[..., :3] * f32(n_a / n) * (f32(0.5) + rng.random((h, w, 3), dtype=f32))
    return base, state, half


def edges(w, h, n_a, n_b, rot: int = 0):
    """The ordinary buffers with pixel i overwritten by kind EDGE_KINDS[(i + rot) % len]."""
    base, state, half = ordinary(w, h, n_a, n_b)
    n = n_a + n_b
    inf, nan = f32(np.inf), f32(np.nan)
    st, hf = state.reshape(-1, 4), half.reshape(-1, 4)
    for i in range(w * h):
        kind = EDGE_KINDS[(i + rot) % len(EDGE_KINDS)]
        q = np.asarray([0.25 * (1 + i % 5), 0.5, 0.75 * (1 + i % 3)], f32)
        if kind == "zeros":
            st[i, :3], hf[i, :3] = 0.0, 0.0
        elif kind == "exact":      # state / N and half / nA are q exactly
            st[i, :3], hf[i, :3] = q * f32(n), q * f32(n_a)
        elif kind == "negative":   # 0.01 + (m.r + m.g + m.b) < 0
            st[i, :3], hf[i, :3] = -q * f32(n), q
        elif kind.startswith("state_"):
            st[i, i % 3] = dict(nan=nan, pinf=inf, ninf=-inf)[kind[6:]]
        elif kind.startswith("half_"):
            hf[i, (i + 1) % 3] = dict(nan=nan, pinf=inf, ninf=-inf)[kind[5:]]
        elif kind == "denormal":
            st[i, :3] = np.asarray([1e-40, 2e-41, 0.0], f32)
            hf[i, :3] = np.asarray([5e-41, 3e-42, 1e-45], f32)
        elif kind == "huge":
            st[i, :3], hf[i, :3] = f32(3e38), f32(1e38)
    return base, state, half


def case_model(hostsim: bool, shape, halves, which: str):
    """1: an injected state through rt_progress_load; pixel map, tile map and stats against restate(), bit for
    bit (NaN matching NaN), host and device forms, with and without the maps."""
    w, h = shape
    n_a, n_b = halves
    s = pc.session(hostsim, "cornell")
    rots = range(len(EDGE_KINDS)) if which == "edge" and w * h < len(EDGE_KINDS) else (0,)
    for rot in rots:
        base, state, half = ordinary(w, h, n_a, n_b) if which == "ordinary" else edges(w, h, n_a, n_b, rot)
        blob = pack_v2(base, state, half, total=n_a + n_b + 2, done=n_a + n_b, passes=2, n_a=n_a)
        assert pc.load_rc(s, blob) == RT_OK, s.where(f"rt_progress_load of the injected state: {s.error()}")
        want = restate(state, half, n_a, n_b, THRESHOLD, 2)
        if which == "ordinary":
            assert want[2]["nonfinite"] == 0 and np.isfinite(want[0]).all(), "the ordinary input has a non-finite pixel"
            assert (want[0] > 0).any() or w * h == 0
        elif w * h >= len(EDGE_KINDS):
            assert want[2]["nonfinite"] >= 7, "the edge input's non-finite pixels"
        msg = s.where(f"{w}x{h} ({n_a}, {n_b}) {which} rot {rot}")
        assert_noise(noise(s), want, msg)
        assert_noise(noise(s, device=True), want, msg + " device form")
        assert_noise(noise(s, maps=False), (None, None, want[2]), msg + " without maps")
        assert_noise(noise(s, device=True, maps=False), (None, None, want[2]), msg + " device form without maps")
        for thr in (0.0, float(want[2]["max_tile"]) if np.isfinite(want[2]["max_tile"]) else 1.0):
            assert_noise(noise(s, thr, maps=False), (None, None, restate(state, half, n_a, n_b, thr, 2)[2]),
                         msg + f" threshold {thr}")
        assert pc.save(s) == blob, s.where("a noise query changed the state")
    s.close()


# ------------------------------------------------------------------ renders
def tracked_run(s, split, noise_between: bool = False, device: bool = False, **kw):
    """A tracked progression over the split; the checkpoint after every pass."""
    pc.begin(s, total=sum(split), **kw)
    track(s)
    blobs = []
    for p, k in enumerate(split):
        pc.advance(s, k)
        if noise_between and p >= 1:
            noise(s, device=device)
        blobs.append(parse(pc.save(s)))
    return blobs


def case_fold(hostsim: bool, scene: str, split):
    """2: half read back through rt_progress_save after every pass against the numpy fold of the states saved
    after each pass; gfx950's words against the hostsim build's."""
    s = pc.session(hostsim, scene)
    cps = tracked_run(s, split)
    hs = None if hostsim else tracked_run(pc.session(True, scene), split)
    for p, cp in enumerate(cps):
        assert (cp["version"], cp["passes"], cp["done"]) == (2, p + 1, sum(split[:p + 1])), s.where(f"header after pass {p}")
        assert cp["n_a"] == sum(split[:p + 1:2]), s.where(f"nA after pass {p}")
        assert_bits(cp["half"], numpy_fold([c["state"] for c in cps[:p + 1]]), s.where(f"{scene} {split}: half after pass {p}"))
        assert (cp["half"][..., 3] == 0).all(), s.where("half's fourth word")
        if hs:
            assert_bits(cp["half"], hs[p]["half"], s.where(f"{scene} {split}: half after pass {p} vs the hostsim build"))
            assert_bits(cp["state"], hs[p]["state"], s.where(f"{scene} {split}: state after pass {p} vs the hostsim build"))
    # the estimate on the rendered state is the restatement's too
    last = cps[-1]
    n_a = last["n_a"]
    assert_noise(noise(s), restate(last["state"], last["half"], n_a, last["done"] - n_a, THRESHOLD, len(split)),
                 s.where(f"{scene} {split}: the estimate on the rendered state"))
    s.close()


def case_same_frame(hostsim: bool, split, device: bool):
    """3: with tracking on, and noise queries between the passes, the resolves are the untracked progression's
    and rt_render's, bit for bit."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    plain = pc.run_split(s, split, base=base)
    plain_lin = dc.resolve_linear(s)
    tracked_run(s, split, noise_between=True, device=device, base=base)
    before = pc.resolve(s, device=device)
    noise(s, device=device)
    assert_bits(pc.resolve(s, device=device), before, s.where("resolves before and after a noise query"))
    assert_bits(before, plain, s.where(f"{split}: tracked vs untracked, rt_progress_resolve"))
    assert_bits(dc.resolve_linear(s, device=device), plain_lin, s.where(f"{split}: tracked vs untracked, linear"))
    assert_bits(before, s.render(W, H, N, NB, base), s.where(f"{split}: tracked vs rt_render"))
    assert_bits(plain_lin, dc.render_linear(s, fb=base), s.where(f"{split}: vs rt_render_linear"))
    s.close()


def case_checkpoint(hostsim: bool):
    """4: save after pass 2 of [3, 1, 2], load in a fresh context, finish: the noise outputs and the frame are
    the uninterrupted run's; an untracked save is version 1; a version-1 load is untracked; bad version-2
    buffers are refused."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    pc.begin(s, base=base)
    track(s)
    pc.advance(s, 3)
    pc.advance(s, 1)
    blob = pc.save(s)
    assert len(blob) == HEADER2 + 3 * 16 * W * H, "a tracked checkpoint's size"
    assert struct.unpack("<12i", blob[:HEADER2])[1:] == (2, W, H, N, 4, NB, 0, 1, H, 2, 3), "the version-2 header"
    pc.advance(s, 2)
    want, frame = noise(s), pc.resolve(s)
    end = pc.save(s)

    t = pc.session(hostsim, "cornell")
    assert pc.load_rc(t, blob) == RT_OK, t.where(f"rt_progress_load (version 2): {t.error()}")
    assert pc.save(t) == blob, "save -> load -> save (version 2)"
    assert track_rc(t) == RT_OK, t.where("rt_progress_noise_track on a loaded tracked progression is harmless")
    pc.advance(t, 2)
    assert_noise(noise(t), want, t.where("the estimate after a resume"))
    assert_bits(pc.resolve(t), frame, t.where("the frame after a resume"))
    assert pc.save(t) == end, "the checkpoint after a resume"
    assert_bits(frame, pc.oracle_frame(t, "cornell", N, "random"), t.where("the tracked frame vs the oracle"))

    # untracked: version 1, today's size; loading it gives an untracked progression
    pc.begin(s, base=base)
    pc.advance(s, 3)
    pc.advance(s, 1)
    v1 = pc.save(s)
    assert len(v1) == pc.HEADER + 2 * 16 * W * H and struct.unpack("<2i", v1[:8]) == (MAGIC, 1), "an untracked save"
    assert v1[pc.HEADER:] == blob[HEADER2:HEADER2 + 2 * 16 * W * H], "base and state do not depend on tracking"
    assert pc.load_rc(t, v1) == RT_OK
    assert noise_rc(t) == RT_ERR_STATE and "tracked" in t.error(), t.where("a version-1 load is untracked")
    assert track_rc(t) == RT_ERR_STATE, t.where("tracking a loaded progression with samples done")

    def v2(passes=2, n_a=3, done=4, cut=0, pad=0):
        words = list(struct.unpack("<12i", blob[:HEADER2]))
        words[5], words[10], words[11] = done, passes, n_a
        body = blob[HEADER2:len(blob) - cut] + b"\0" * pad
        return struct.pack("<12i", *words) + body

    assert pc.load_rc(t, v2()) == RT_OK, t.where(f"the rebuilt checkpoint: {t.error()}")
    for what, bad in (("truncated", v2(cut=16)), ("one buffer short", v2(cut=16 * W * H)), ("long", v2(pad=16)),
                      ("nA > done", v2(n_a=5)), ("nA < 0", v2(n_a=-1)), ("passes < 0", v2(passes=-1)),
                      ("header only", blob[:HEADER2]), ("version-1 size", blob[:pc.HEADER] + blob[HEADER2:HEADER2 + 2 * 16 * W * H]),
                      ("version 3", struct.pack("<2i", MAGIC, 3) + blob[8:])):
        assert pc.load_rc(t, bad) == RT_ERR_ARG and t.error(), t.where(f"bad version-2 checkpoint: {what}")
    assert pc.info(t)[3] == 4 and noise_rc(t) == RT_OK, t.where("a refused load left the progression alone")
    s.close()
    t.close()


def case_shard(hostsim: bool):
    """5: rows 1::2: tiles are over the shard's local rows; a rendered and an injected shard state."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    cps = tracked_run(s, [3, 1, 2], base=base, off=1, stride=2)
    last = cps[-1]
    rows = (H - 1 + 1) // 2
    assert last["rows"] == rows and last["state"].shape == (rows, W, 4)
    got = noise(s)
    assert got[1].shape == ((rows + 7) // 8, (W + 7) // 8)
    assert_noise(got, restate(last["state"], last["half"], 5, 1, THRESHOLD, 3), s.where("the shard's estimate"))
    assert_noise(noise(s, device=True), restate(last["state"], last["half"], 5, 1, THRESHOLD, 3), s.where("device form"))
    assert_bits(pc.resolve(s), pc.oracle_frame(s, "cornell", N, "random")[1::2], s.where("the shard's frame vs the oracle"))
    b, st, hf = edges(W, rows, 2, 4)
    blob = pack_v2(b, st, hf, total=N, done=N, passes=2, n_a=2, h=H, off=1, stride=2)
    assert pc.load_rc(s, blob) == RT_OK, s.where(f"an injected shard: {s.error()}")
    assert_noise(noise(s), restate(st, hf, 2, 4, THRESHOLD, 2), s.where("an injected shard state"))
    s.close()


def case_errors(hostsim: bool):
    """6: the state and argument errors; tracking dropped by every rebind that ends a progression."""
    s = pc.session(hostsim, "cornell")
    st = NoiseStats()
    assert track_rc(s) == RT_ERR_STATE and s.error(), s.where("track without a progression")
    assert noise_rc(s) == RT_ERR_STATE, s.where("noise without a progression")
    assert s.L.rt_progress_noise_track(None) == RT_ERR_ARG and s.L.rt_progress_noise(None, 0.1, ctypes.byref(st), None, None) == RT_ERR_ARG
    pc.begin(s)
    pc.advance(s, 1)
    assert track_rc(s) == RT_ERR_STATE and "done" in s.error(), s.where("track after a pass")
    assert noise_rc(s) == RT_ERR_STATE and "tracked" in s.error(), s.where("noise on an untracked progression")
    pc.begin(s)
    track(s)
    track(s)  # (a second call is harmless)
    assert noise_rc(s) == RT_ERR_STATE, s.where("noise before any pass")
    pc.advance(s, 2)
    assert noise_rc(s) == RT_ERR_STATE and "both halves" in s.error(), s.where("noise after one pass only")
    assert s.L.rt_progress_noise_device(s.ctx, 0.1, _capi.ptr(np.zeros(8, np.int32)), None, None, None) == RT_ERR_STATE
    track(s)  # (still harmless once tracked)
    pc.advance(s, 1)
    assert noise_rc(s) == RT_OK, s.where(f"noise after two passes: {s.error()}")
    for thr in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert noise_rc(s, thr) == RT_ERR_ARG and "threshold" in s.error(), s.where(f"threshold {thr}")
        assert s.L.rt_progress_noise_device(s.ctx, thr, _capi.ptr(np.zeros(8, np.int32)), None, None, None) == RT_ERR_ARG
    assert noise_rc(s, 0.0) == RT_OK and noise_rc(s, -0.0) == RT_OK, s.where("threshold 0")
    assert noise_rc(s, stats=False) == RT_ERR_ARG and "stats" in s.error(), s.where("stats NULL")
    assert s.L.rt_progress_noise_device(s.ctx, 0.1, None, None, None, None) == RT_ERR_ARG, s.where("d_stats NULL")
    odd = np.zeros(40, np.uint8)[1:33]
    assert s.L.rt_progress_noise_device(s.ctx, 0.1, _capi.ptr(odd), None, None, None) == RT_ERR_ARG and "aligned" in s.error()
    # an advance with nothing left is no pass
    pc.advance(s, 100)
    before = noise(s)[2]
    pc.advance(s, 1)
    assert noise(s)[2] == before and before["passes"] == 3, s.where("an idle advance counted as a pass")
    # every rebind ends the progression and its tracking
    for name, call in pc._rebinds(s).items():
        pc.begin(s)
        track(s)
        pc.advance(s, 1)
        pc.advance(s, 1)
        assert noise_rc(s) == RT_OK
        call()
        assert noise_rc(s) == RT_ERR_STATE and track_rc(s) == RT_ERR_STATE, s.where(f"after {name}")
        pc.begin(s)
        pc.advance(s, 1)
        pc.advance(s, 1)
        assert noise_rc(s) == RT_ERR_STATE and "tracked" in s.error(), s.where(f"a new progression after {name} is untracked")
    pc.begin(s)
    track(s)
    s.L.rt_progress_end(s.ctx)
    assert track_rc(s) == RT_ERR_STATE, s.where("after rt_progress_end")
    s.close()
    # a multi-device context has no progression to track (hostsim: two host "devices"; gfx950: loopback)
    m = Session(hostsim, name="noise-multi", devices=[0, 1] if hostsim else [0, 0], loopback=not hostsim)
    pc.bind(m, "cornell")
    assert pc.begin_rc(m) == RT_ERR_ARG and "multi-device" in m.error(), "rt_progress_begin on a multi-device context"
    assert track_rc(m) == RT_ERR_STATE and noise_rc(m) == RT_ERR_STATE, "noise calls on a multi-device context"
    blob = pack_v2(*ordinary(8, 8, 1, 1), total=4, done=2, passes=2, n_a=1)
    assert pc.load_rc(m, blob) == RT_ERR_ARG, "a version-2 load on a multi-device context"
    m.close()


def case_measures_noise(hostsim: bool):
    """7: cornell, 40x30: the mean tile error at 64 samples ([32, 32]) is strictly less than at 4 ([2, 2]).
    Measured on the hostsim build: 0.27372 at 4 and 0.10117 at 64 (ratio 2.7; 1 / sqrt(16) would give 4)."""
    s = pc.session(hostsim, "cornell")
    means = []
    for split in ([2, 2], [32, 32]):
        tracked_run(s, split)
        _, tile, st = noise(s)
        assert st["nonfinite"] == 0 and (st["samples_a"], st["samples_b"]) == (split[0], split[1])
        means.append(float(tile.astype(np.float64).mean()))
    print(f"mean tile error: {means[0]:.6g} at 4 samples, {means[1]:.6g} at 64, ratio {means[0] / means[1]:.3f}")
    assert means[1] < means[0], f"the estimate did not fall with the sample count: {means}"
    s.close()


def case_python(hostsim: bool):
    """8: RenderKernel.progress_track_noise / progress_noise agree with the C ABI."""
    import rt_amd
    from conftest import parsed_scene
    P = parsed_scene("cornell")
    img = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, N, NB, img, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices,
                             None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sc.rt_cases.sky("S")), None, device=0,
                             hostsim=hostsim)
    cam = sc.camera_of("cornell")
    rk.set_camera(rt_amd.Camera(cam[:16].reshape(4, 4), float(cam[16])))
    rk.progress_begin()
    rk.progress_track_noise()
    rk.progress_advance(3)
    try:
        rk.progress_noise(THRESHOLD)
        raise AssertionError("progress_noise after one pass did not raise")
    except rt_amd.RtError as e:
        assert "both halves" in str(e)
    rk.progress_advance(1)
    s = pc.session(hostsim, "cornell")
    pc.begin(s, total=N)
    track(s)
    pc.advance(s, 3)
    pc.advance(s, 1)
    px, tl, st = noise(s)
    got = rk.progress_noise(THRESHOLD, pixel_map=True, tile_map=True)
    assert set(got) == set(STAT_KEYS) | {"pixel_err", "tile_err"}
    assert_noise((got["pixel_err"], got["tile_err"], got), (px, tl, st), "RenderKernel.progress_noise vs the C ABI")
    plain = rk.progress_noise(THRESHOLD)
    assert set(plain) == set(STAT_KEYS) and plain == {k: got[k] for k in STAT_KEYS}
    blob = rk.progress_save()
    assert struct.unpack("<2i", blob[:8]) == (MAGIC, 2)
    rk.progress_end()
    s.close()
