"""Adaptive progressions (rt_progress_advance_adaptive, rt_progress_tile_counts, checkpoint version 3;
include/rt_hip.h). The reference of the selection is restated here in numpy float32 and never calls the
library: noise_cases.restate generalised to per-tile counts, then the active and capped rules, the prefix
sums and the count updates. The reference of the rendered pixels is the library's own untracked uniform
progression (itself held to the oracle by progress_cases): a pixel with c samples must hold, bit for bit,
what that progression holds at done = c.

Frames are progress_cases' 40x30, 4 bounces, total 8, passes of 1 or 2 samples, except the selection's
shapes. Shared by tests/test_adapt.py (hostsim) and tests/test_adapt_gpu.py (gfx950).

Helpers only: no tests here."""
from __future__ import annotations

import ctypes
import struct

import numpy as np

import display_cases as dc
import noise_cases as nc
import progress_cases as pc
import session_cases as sc
from noise_cases import MAGIC, f32
from progress_cases import H, NB, W
from session_cases import Session, assert_bits

from rt_amd import _capi
from rt_amd._capi import RT_ERR_ARG, RT_ERR_STATE, RT_OK

TOTAL = 8
# 264x264 is 33x33 = 1,089 tiles: more than one step of k_adapt_select's 1,024-thread scan (rt_adapt.hip)
SHAPES = ((1, 1), (8, 8), (9, 1), (1, 9), (17, 9), (40, 30), (64, 8), (264, 264))  # (w, h)
INFO_KEYS = ("active_tiles", "active_pixels", "capped_tiles", "min_count", "max_count", "tiles")
HEADER2 = pc.HEADER + 8
# the wave plans of a pixel-list pass (rt_test_schedule): lanes 1 / 3 / 4, tail on or off, fast lane on or off
SCHEDULES = dict(default={}, lanes1_notail=dict(lanes=1, tail_paths=0), lanes3_tail=dict(lanes=3, tail_paths=1, tail_enter=1000),
                 lanes4_fast=dict(lanes=4, fast_k=64, fast_spp=0.0))


# ------------------------------------------------------------------ the reference (numpy float32)
def expand(a, rows, w):
    """A per-tile array [th, tw] as a per-pixel one [rows, w]."""
    return np.repeat(np.repeat(np.asarray(a), 8, 0), 8, 1)[:rows, :w]


def tile_counts_px(rows, w):
    th, tw = (rows + 7) // 8, (w + 7) // 8
    return np.minimum(8, w - 8 * np.arange(tw))[None, :] * np.minimum(8, rows - 8 * np.arange(th))[:, None]


def restate(state, half, tn, tna, threshold: float, n_a: int, n_b: int, passes: int):
    """noise_cases.restate with every tile's own counts: (pixel_err, tile_err, stats)."""
    state, half = np.asarray(state, f32), np.asarray(half, f32)
    rows, w = state.shape[:2]
    n = expand(tn, rows, w).astype(f32)
    na = expand(tna, rows, w).astype(f32)
    nb = expand(np.asarray(tn) - np.asarray(tna), rows, w).astype(f32)
    with np.errstate(all="ignore"):
        k = np.sqrt(na / nb)
        m, a = state[..., :3] / n[..., None], half[..., :3] / na[..., None]
        d = (np.abs(m[..., 0] - a[..., 0]) + np.abs(m[..., 1] - a[..., 1])) + np.abs(m[..., 2] - a[..., 2])
        e = (k * d) / np.sqrt(f32(0.01) + ((m[..., 0] + m[..., 1]) + m[..., 2]))
    assert e.dtype == f32 and k.dtype == f32
    th, tw = (rows + 7) // 8, (w + 7) // 8
    fin = np.isfinite(e)
    pad = np.zeros((th * 8, tw * 8), f32)
    pad[:rows, :w] = np.where(fin, e, f32(0.0))
    v = pad.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(th, tw, 64)
    with np.errstate(all="ignore"):
        for _ in range(6):
            v = v[..., 0::2] + v[..., 1::2]
        tile = v[..., 0] / tile_counts_px(rows, w).astype(f32)
    assert tile.dtype == f32
    stats = dict(tiles=th * tw, tiles_over=int((tile > f32(threshold)).sum()), nonfinite=int((~fin).sum()),
                 max_tile=f32(tile.max()), samples_a=n_a, samples_b=n_b, passes=passes)
    return e, tile, stats


def select(tile_err, tn, tna, s: int, total: int, threshold: float, passes: int, rows: int, w: int):
    """The rules of a pass: (active [th, tw] bool, info dict, tile_n after, tile_nA after, tile_off of the
    active tiles in ascending t)."""
    tn, tna = np.asarray(tn, np.int64), np.asarray(tna, np.int64)
    fits = tn + s <= total
    over = np.ones(tn.shape, bool) if passes < 2 else (np.asarray(tile_err, f32) > f32(threshold))  # (NaN: False)
    active = fits & over
    capped = (~fits & over) if passes >= 2 else np.zeros(tn.shape, bool)
    px = np.where(active, tile_counts_px(rows, w), 0).reshape(-1)
    off = (np.cumsum(px) - px)[active.reshape(-1)]
    a_pass = passes % 2 == 0
    tn2 = tn + np.where(active, s, 0)
    tna2 = tna + np.where(active & a_pass, s, 0)
    info = dict(active_tiles=int(active.sum()), active_pixels=int(px.sum()), capped_tiles=int(capped.sum()),
                min_count=int(tn2.min()), max_count=int(tn2.max()), tiles=int(tn.size))
    return active, info, tn2.astype(np.int32), tna2.astype(np.int32), off


def masked_fold(states, masks):
    """noise_cases.numpy_fold with the passes' active pixel masks ([rows, w] bool): only active pixels fold."""
    half = np.zeros_like(states[0])
    prev = np.zeros_like(states[0])
    with np.errstate(all="ignore"):
        for p, (st, mk) in enumerate(zip(states, masks)):
            if p % 2 == 0:
                h = half[..., :3] - prev[..., :3]
                h = h + st[..., :3]
                half[..., :3] = np.where(mk[..., None], h, half[..., :3])
            prev = st
    return half


# ------------------------------------------------------------------ checkpoints
def pack_v3(base, state, half, tn, tna, total, passes, n_a, n_b, h=None, off=0, stride=1, nb=NB, version=3) -> bytes:
    rows, w = state.shape[:2]
    h = rows if h is None else h
    head = struct.pack("<10i", MAGIC, version, w, h, total, n_a + n_b, nb, off, stride, rows) + struct.pack("<2i", passes, n_a)
    body = b"".join(np.ascontiguousarray(a, f32).tobytes() for a in (base, state, half))
    return head + body + b"".join(np.ascontiguousarray(a, np.int32).tobytes() for a in (tn, tna))


def parse(blob: bytes) -> dict:
    hd = struct.unpack("<10i", blob[:pc.HEADER])
    w, rows, version = hd[2], hd[9], hd[1]
    out = dict(version=version, w=w, h=hd[3], total=hd[4], done=hd[5], rows=rows)
    assert version in (2, 3), f"a tracked checkpoint's version: {version}"
    out["passes"], out["n_a"] = struct.unpack("<2i", blob[pc.HEADER:HEADER2])
    n = rows * w * 16
    th, tw = (rows + 7) // 8, (w + 7) // 8
    assert len(blob) == HEADER2 + 3 * n + (8 * th * tw if version == 3 else 0), "the checkpoint's size"
    for i, k in enumerate(("base", "state", "half")):
        out[k] = np.frombuffer(blob[HEADER2 + i * n:HEADER2 + (i + 1) * n], f32).reshape(rows, w, 4)
    if version == 3:
        cnt = np.frombuffer(blob[HEADER2 + 3 * n:], np.int32)
        out["tile_n"], out["tile_nA"] = cnt[:th * tw].reshape(th, tw), cnt[th * tw:].reshape(th, tw)
    return out


# ------------------------------------------------------------------ the calls
def advance_rc(s, k, threshold, info=True):
    out = np.full(8, -7, np.int32)
    rc = s.L.rt_progress_advance_adaptive(s.ctx, k, threshold, None, _capi.ptr(out) if info else None)
    return rc, out


def advance(s, k, threshold) -> dict:
    rc, out = advance_rc(s, k, threshold)
    s.ok(rc, f"rt_progress_advance_adaptive({k}, {threshold})")
    assert int(out[6]) == 0 and int(out[7]) == 0, s.where("info words 6 and 7")
    return {k_: int(v) for k_, v in zip(INFO_KEYS, out)}


def counts(s):
    i = pc.info(s)
    shape = ((i[7] + 7) // 8, (i[0] + 7) // 8)
    n, na = np.full(shape, -3, np.int32), np.full(shape, -3, np.int32)
    s.ok(s.L.rt_progress_tile_counts(s.ctx, _capi.ptr(n), _capi.ptr(na)), "rt_progress_tile_counts")
    only = np.full(shape, -3, np.int32)
    s.ok(s.L.rt_progress_tile_counts(s.ctx, None, _capi.ptr(only)), "rt_progress_tile_counts(NULL, nA)")
    assert (only == na).all()
    return n, na


# ------------------------------------------------------------------ 1: the selection, by injected state
def injected_counts(w, h, total, s):
    """Random per-tile counts with nA = 0, nB = 0, n = total, n + s = total + 1 and n + s = total among them."""
    th, tw = (h + 7) // 8, (w + 7) // 8
    rng = np.random.default_rng([nc.SEED, w, h, 77])
    tn = rng.integers(2, total + 1, (th, tw)).astype(np.int32)
    tna = np.minimum(tn - 1, rng.integers(1, total, (th, tw))).astype(np.int32)
    flat_n, flat_a = tn.reshape(-1), tna.reshape(-1)
    special = ((2, 0), (3, 3), (total, 1), (total - s + 1, 1), (total - s, 2))
    for i in range(0, flat_n.size, 3):  # every third tile takes the next special pair
        flat_n[i], flat_a[i] = special[(i // 3) % len(special)]
    return tn, tna


def case_select(hostsim: bool, shape, which: str, s_pass: int = 1):
    """1: an injected state through a version-3 rt_progress_load, then one adaptive pass of one sample at the
    threshold `which`: info, the tile counts and a saved checkpoint's count arrays against select(), exactly;
    pixels of inactive tiles untouched in state and half, bit for bit."""
    w, h = shape
    total = 6
    s = pc.session(hostsim, "cornell")
    rots = range(min(len(nc.EDGE_KINDS), 3)) if w * h < len(nc.EDGE_KINDS) else (0,)
    for rot in rots:
        base, state, half = nc.edges(w, h, 2, 2, rot)
        tn, tna = injected_counts(w, h, total, s_pass)
        if w * h == 1:
            tn[:], tna[:] = ((2, 1), (total, 1), (3, 0))[rot]
        _, tile, _ = restate(state, half, tn, tna, 0.0, 2, 2, 2)
        fin = tile[np.isfinite(tile)]
        thr = dict(zero=0.0, median=float(np.median(fin)) if fin.size else 0.5,
                   above=float(fin.max()) + 1.0 if fin.size else 1.0)[which]
        # (1 bounce: the selection does not depend on what the pass renders)
        blob = pack_v3(base, state, half, tn, tna, total, passes=2, n_a=2, n_b=2, nb=1)
        assert pc.load_rc(s, blob) == RT_OK, s.where(f"rt_progress_load of the injected state: {s.error()}")
        assert pc.save(s) == blob, s.where("save -> load -> save (version 3)")
        got_n, got_na = counts(s)
        assert (got_n == tn).all() and (got_na == tna).all(), s.where("the loaded counts")
        assert pc.info(s)[3] == int(tn.min()), s.where("rt_progress_info's done is the smallest tile count")
        msg = s.where(f"{w}x{h} threshold {which} = {thr} rot {rot}")
        # the noise query of the adaptive progression is the per-tile restatement
        want_noise = restate(state, half, tn, tna, thr, 2, 2, 2)
        nc.assert_noise(nc.noise(s, thr), want_noise, msg + " noise, host form")
        nc.assert_noise(nc.noise(s, thr, device=True), want_noise, msg + " noise, device form")
        active, want, tn2, tna2, _ = select(tile, tn, tna, s_pass, total, thr, 2, h, w)
        if which == "above":
            assert want["active_tiles"] == 0
        got = advance(s, s_pass, thr)
        assert got == want, f"{msg}: info {got} != {want}"
        got_n, got_na = counts(s)
        assert (got_n == tn2).all(), f"{msg}: tile_n\n{got_n}\n{tn2}"
        assert (got_na == tna2).all(), f"{msg}: tile_nA\n{got_na}\n{tna2}"
        cp = parse(pc.save(s))
        assert (cp["tile_n"] == tn2).all() and (cp["tile_nA"] == tna2).all(), f"{msg}: the saved counts"
        assert cp["passes"] == (3 if want["active_tiles"] else 2), f"{msg}: passes {cp['passes']}"
        assert cp["n_a"] == (2 + s_pass if want["active_tiles"] else 2) and cp["done"] - cp["n_a"] == 2, f"{msg}: nA, nB"
        apx = expand(active, h, w)
        assert_bits(cp["state"][~apx], state[~apx], msg + ": state of inactive pixels")
        assert_bits(cp["half"][~apx], half[~apx], msg + ": half of inactive pixels")
        assert_bits(cp["base"], base, msg + ": base")
        if apx.any():  # every active pixel drew a sample: its RNG word moved
            moved = cp["state"][..., 3].view(np.uint32) != state[..., 3].view(np.uint32)
            assert moved[apx].all(), f"{msg}: {int((~moved[apx]).sum())} active pixels did not advance"
    s.close()


# ------------------------------------------------------------------ 2, 3: chain identity and the fold
def uniform_refs(hostsim: bool, scene: str, total: int, cs, base=None, **kw) -> dict:
    """c -> (state, resolve, linear resolve) of an untracked uniform progression of `total` at done = c."""
    s = pc.session(hostsim, scene)
    out = {}
    for c in cs:
        pc.begin(s, total=total, base=base, **kw)
        pc.advance(s, c)
        blob = pc.save(s)
        rows, w = pc.info(s)[7], pc.info(s)[0]
        st = np.frombuffer(blob[pc.HEADER + 16 * rows * w:], f32).reshape(rows, w, 4)
        out[c] = (st, pc.resolve(s), dc.resolve_linear(s))
    s.close()
    return out


def adaptive_run(s, total=TOTAL, step=2, base=None, stop_after=None, resume: bytes | None = None, **kw):
    """Track, [2, 2] uniformly, T = the median of the finite tile errors, then adaptive passes of `step` until
    none is active. Returns dict(T, blobs (parsed checkpoint after every pass), masks (per-pixel, per pass),
    infos). resume: a checkpoint of this run to go on from (with its T in kw['T'])."""
    T = kw.pop("T", None)
    blobs, masks, infos = [], [], []
    if resume is None:
        pc.begin(s, total=total, base=base, **kw)
        nc.track(s)
        rows, w = pc.info(s)[7], pc.info(s)[0]
        for _ in range(2):
            pc.advance(s, 2)
            blobs.append(nc.parse(pc.save(s)))
            masks.append(np.ones((rows, w), bool))
        tile = nc.noise(s)[1]
        T = float(np.median(tile[np.isfinite(tile)]))
    else:
        assert pc.load_rc(s, resume) == RT_OK, s.where(f"rt_progress_load (version 3): {s.error()}")
        rows, w = pc.info(s)[7], pc.info(s)[0]
    while True:
        before = counts(s)[0]
        i = advance(s, step, T)
        infos.append(i)
        if i["active_tiles"] == 0:
            break
        blobs.append(parse(pc.save(s)))
        masks.append(expand(counts(s)[0] != before, rows, w))
        if stop_after is not None and len(infos) == stop_after:
            break
    return dict(T=T, blobs=blobs, masks=masks, infos=infos)


def case_chain(hostsim: bool, scene: str = "cornell", step: int = 2, off: int = 0, stride: int = 1, schedule=None,
               against_hostsim: bool = False):
    """2, 3 (and 6 with against_hostsim): every pixel is the untracked uniform progression's at its tile's count
    (state words, tone-mapped and linear resolve, bit for bit), the seed-31 line is the oracle's c-sample frame,
    half is the masked fold of the saved states, and the noise query is the per-tile restatement."""
    s = pc.session(hostsim, scene, schedule=schedule)
    kw = dict(off=off, stride=stride) if (off, stride) != (0, 1) else {}
    run = adaptive_run(s, step=step, **kw)
    msg = s.where(f"{scene} step {step} shard {off}::{stride}")
    first = run["infos"][0]
    n_tiles = first["tiles"]
    print(f"T = {run['T']:.6g}; passes: {[i['active_tiles'] for i in run['infos']]} of {n_tiles} tiles")
    assert first["active_tiles"] >= n_tiles / 4 and n_tiles - first["active_tiles"] >= n_tiles / 4, \
        f"{msg}: the first adaptive pass has {first['active_tiles']} of {n_tiles} tiles active"
    assert run["infos"][-1]["active_tiles"] == 0
    tn, tna = counts(s)
    last = run["blobs"][-1]
    rows, w = last["rows"], last["w"]
    assert (last["tile_n"] == tn).all() and (last["tile_nA"] == tna).all() and last["version"] == 3
    assert pc.info(s)[3] == tn.min()
    cs = sorted(set(int(c) for c in tn.reshape(-1)))
    assert len(cs) >= 2 and max(cs) <= TOTAL, f"{msg}: counts {cs}"
    got_res, got_lin = pc.resolve(s), dc.resolve_linear(s)
    assert_bits(pc.resolve(s, device=True), got_res, msg + ": device resolve")
    assert_bits(dc.resolve_linear(s, device=True), got_lin, msg + ": device linear resolve")
    refs = uniform_refs(hostsim, scene, TOTAL, cs, **kw)
    cpx = expand(tn, rows, w)
    ys = (off + stride * np.arange(rows))[:, None] * np.ones((1, w), int)
    line = (ys * np.arange(w)[None, :]) == 0
    for c in cs:
        m = cpx == c
        st, res, lin = refs[c]
        assert_bits(last["state"][m], st[m], f"{msg}: state of the tiles at {c} samples vs the uniform progression")
        assert_bits(got_res[m], res[m], f"{msg}: resolve of the tiles at {c} samples")
        assert_bits(got_lin[m], lin[m], f"{msg}: linear resolve of the tiles at {c} samples")
        if scene in ("cornell", "fan") and (m & line).any():
            want = pc.oracle_frame(s, scene, c)[off::stride]
            assert_bits(got_res[m & line], want[m & line], f"{msg}: the seed-31 line at {c} samples vs the oracle")
    if TOTAL in cs:
        full = s.render(W, H, TOTAL, NB)[off::stride]
        assert_bits(got_res[cpx == TOTAL], full[cpx == TOTAL], msg + ": tiles at the total vs rt_render")
    # 3: the fold under the masks, from the states saved after each pass
    for p, cp in enumerate(run["blobs"]):
        want = masked_fold([b["state"] for b in run["blobs"][:p + 1]], run["masks"][:p + 1])
        assert_bits(cp["half"], want, f"{msg}: half after pass {p}")
    n_pass = len(run["blobs"])
    n_a = 2 + step * len(range(2, n_pass, 2))
    n_b = 2 + step * len(range(3, n_pass, 2))
    assert (last["passes"], last["n_a"], last["done"]) == (n_pass, n_a, n_a + n_b), f"{msg}: the header's pass words"
    want = restate(last["state"], last["half"], tn, tna, run["T"], n_a, n_b, n_pass)
    nc.assert_noise(nc.noise(s, run["T"]), want, msg + ": noise, host form")
    nc.assert_noise(nc.noise(s, run["T"], device=True), want, msg + ": noise, device form")
    if against_hostsim:
        hs = pc.session(True, scene)
        ref = adaptive_run(hs, step=step, **kw)
        assert ref["infos"] == run["infos"] and ref["T"] == run["T"], f"{msg}: the passes vs the hostsim build"
        for p, (a, b) in enumerate(zip(run["blobs"], ref["blobs"])):
            for k in ("state", "half") + (("tile_n", "tile_nA") if a["version"] == 3 else ()):
                assert_bits(a[k], b[k], f"{msg}: {k} after pass {p} vs the hostsim build")
        assert_bits(got_res, pc.resolve(hs), msg + ": resolve vs the hostsim build")
        hs.close()
    s.close()


# ------------------------------------------------------------------ 4: the checkpoint
def case_checkpoint(hostsim: bool):
    """4: save after the first adaptive pass, load in a fresh context, continue: the final checkpoint (state, half,
    counts) and the resolves are the uninterrupted run's; versions 1 and 2 round-trip to identical bytes; bad
    version-3 buffers are refused."""
    s = pc.session(hostsim, "cornell")
    base = pc.base_of("random")
    whole = adaptive_run(s, base=base)
    end, frame, lin = pc.save(s), pc.resolve(s), dc.resolve_linear(s)
    part = adaptive_run(s, base=base, stop_after=1)
    assert part["T"] == whole["T"]
    blob = pc.save(s)
    assert struct.unpack("<2i", blob[:8]) == (MAGIC, 3)
    assert len(blob) == HEADER2 + 3 * 16 * W * H + 2 * 4 * 20, "a version-3 checkpoint's size"
    t = pc.session(hostsim, "cornell")
    rest = adaptive_run(t, resume=blob, T=part["T"])
    assert rest["infos"] == whole["infos"][1:], t.where("the passes after a resume")
    assert pc.save(t) == end, t.where("the checkpoint after a resume")
    assert_bits(pc.resolve(t), frame, t.where("the frame after a resume"))
    assert_bits(dc.resolve_linear(t), lin, t.where("the linear frame after a resume"))
    if not hostsim:  # the gfx950 run's checkpoints against the hostsim build's, word for word
        hs = pc.session(True, "cornell")
        hs_whole = adaptive_run(hs, base=base)
        assert hs_whole["infos"] == whole["infos"] and hs_whole["T"] == whole["T"], s.where("the passes vs the hostsim build")
        assert pc.save(hs) == end, s.where("the final checkpoint vs the hostsim build")
        adaptive_run(hs, base=base, stop_after=1)
        assert pc.save(hs) == blob, s.where("the checkpoint after the first adaptive pass vs the hostsim build")
        hs.close()
    # versions 1 and 2 as before
    pc.begin(s, base=base)
    pc.advance(s, 3)
    v1 = pc.save(s)
    assert struct.unpack("<2i", v1[:8]) == (MAGIC, 1) and pc.load_rc(t, v1) == RT_OK and pc.save(t) == v1
    pc.begin(s, base=base)
    nc.track(s)
    pc.advance(s, 3)
    pc.advance(s, 1)
    v2 = pc.save(s)
    assert struct.unpack("<2i", v2[:8]) == (MAGIC, 2) and pc.load_rc(t, v2) == RT_OK and pc.save(t) == v2
    n, na = counts(t)  # (tracked, not adaptive yet: the uniform counts)
    assert (n == 4).all() and (na == 3).all()
    # bad version-3 buffers
    cp = parse(blob)
    nt = cp["tile_n"].size

    def v3(tn=None, tna=None, cut=0, pad=0):
        tn = cp["tile_n"] if tn is None else tn
        tna = cp["tile_nA"] if tna is None else tna
        b = pack_v3(cp["base"], cp["state"], cp["half"], tn, tna, cp["total"], cp["passes"], cp["n_a"], cp["done"] - cp["n_a"])
        return b[:len(b) - cut] + b"\0" * pad

    assert v3() == blob and pc.load_rc(t, blob) == RT_OK
    one = np.zeros_like(cp["tile_n"])
    one.reshape(-1)[nt - 1] = 1
    for what, bad in (("truncated", v3(cut=4)), ("long", v3(pad=4)), ("no count arrays", blob[:len(blob) - 8 * nt]),
                      ("one count array", blob[:len(blob) - 4 * nt]), ("tile_nA > tile_n", v3(tna=cp["tile_n"] + one)),
                      ("tile_nA < 0", v3(tna=cp["tile_nA"] - 9 * one)), ("tile_n > total", v3(tn=cp["tile_n"] + 100 * one)),
                      ("tile_n < 0", v3(tn=cp["tile_n"] - 100 * one, tna=0 * one)),
                      ("zero and positive counts", v3(tn=cp["tile_n"] * (1 - one), tna=cp["tile_nA"] * (1 - one))),
                      ("version 2 with counts", struct.pack("<2i", MAGIC, 2) + blob[8:]),
                      ("version 4", struct.pack("<2i", MAGIC, 4) + blob[8:])):
        assert pc.load_rc(t, bad) == RT_ERR_ARG and t.error(), t.where(f"bad version-3 checkpoint: {what}")
    assert (counts(t)[0] == cp["tile_n"]).all(), t.where("a refused load left the progression alone")
    s.close()
    t.close()


# ------------------------------------------------------------------ 5: errors and state
def case_errors(hostsim: bool):
    s = pc.session(hostsim, "cornell")
    info = np.zeros(8, np.int32)
    assert advance_rc(s, 1, 0.1)[0] == RT_ERR_STATE and s.error(), s.where("no progression")
    assert s.L.rt_progress_tile_counts(s.ctx, None, None) == RT_ERR_STATE, s.where("tile counts without a progression")
    assert s.L.rt_progress_advance_adaptive(None, 1, 0.1, None, _capi.ptr(info)) == RT_ERR_ARG
    assert s.L.rt_progress_tile_counts(None, None, None) == RT_ERR_ARG
    pc.begin(s, total=TOTAL)
    assert advance_rc(s, 1, 0.1)[0] == RT_ERR_STATE and "tracked" in s.error(), s.where("an untracked progression")
    assert s.L.rt_progress_tile_counts(s.ctx, None, None) == RT_ERR_STATE, s.where("tile counts, untracked")
    pc.begin(s, total=TOTAL)
    nc.track(s)
    for k in (0, -1):
        assert advance_rc(s, k, 0.1)[0] == RT_ERR_ARG and "samples" in s.error(), s.where(f"samples {k}")
    for thr in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert advance_rc(s, 1, thr)[0] == RT_ERR_ARG and "threshold" in s.error(), s.where(f"threshold {thr}")
    assert advance_rc(s, 1, 0.1, info=False)[0] == RT_ERR_ARG and "info" in s.error(), s.where("info NULL")
    assert pc.save(s)[4:8] == struct.pack("<i", 2), s.where("a refused call made the progression adaptive")
    # the first two passes take every tile, whatever the threshold; equal counts: the uniform advance still works
    i = advance(s, 2, 1e30)
    assert (i["active_tiles"], i["active_pixels"], i["capped_tiles"], i["min_count"], i["max_count"]) == (20, W * H, 0, 2, 2)
    # (a first pass that is adaptive starts the chains as a uniform one does)
    assert_bits(parse(pc.save(s))["state"], uniform_refs(hostsim, "cornell", TOTAL, [2])[2][0], s.where("an adaptive first pass"))
    assert nc.noise_rc(s) == RT_ERR_STATE, s.where("noise after one pass")
    pc.advance(s, 2)
    n, na = counts(s)
    assert (n == 4).all() and (na == 2).all() and pc.info(s)[3] == 4, s.where("a uniform pass keeps the counts in step")
    _, tile, st = nc.noise(s)
    assert (st["samples_a"], st["samples_b"], st["passes"]) == (2, 2, 2)
    # a threshold above the maximum: no launch, passes unchanged
    before = pc.save(s)
    i = advance(s, 2, float(st["max_tile"]) + 1.0)
    assert i["active_tiles"] == 0 and i["active_pixels"] == 0 and pc.save(s) == before, s.where("no tile above the threshold")
    # renders, queries and rt_denoise between adaptive passes change nothing
    T = float(np.median(tile))
    i = advance(s, 2, T)
    assert 0 < i["active_tiles"] < 20 and i["min_count"] == 4 and i["max_count"] == 6, s.where(f"a pass at the median: {i}")
    before = pc.save(s)
    s.render(W, H, 2, NB)
    s.query(s.rays(64))
    alb, nd = s.features(W, H)
    s.denoise(pc.resolve(s), alb, nd, 2, 1.0)
    nc.noise(s, T)
    counts(s)
    assert pc.save(s) == before, s.where("other calls between adaptive passes changed the progression")
    # the counts differ now: the uniform advance is refused and changes nothing
    assert pc.advance_rc(s, 1) == RT_ERR_STATE and "adaptive" in s.error(), s.where("a uniform advance after the counts diverged")
    assert pc.save(s) == before
    # capped: a pass that no longer fits
    i = advance(s, 3, 0.0)
    assert i["capped_tiles"] > 0 and i["max_count"] <= TOTAL, s.where(f"capped tiles: {i}")
    # every rebind ends the progression
    for name, call in pc._rebinds(s).items():
        pc.begin(s, total=TOTAL)
        nc.track(s)
        advance(s, 1, 0.0)
        call()
        assert advance_rc(s, 1, 0.0)[0] == RT_ERR_STATE, s.where(f"after {name}")
        assert s.L.rt_progress_tile_counts(s.ctx, None, None) == RT_ERR_STATE, s.where(f"tile counts after {name}")
    s.close()
    m = Session(hostsim, name="adapt-multi", devices=[0, 1] if hostsim else [0, 0], loopback=not hostsim)
    pc.bind(m, "cornell")
    assert advance_rc(m, 1, 0.1)[0] == RT_ERR_ARG and "multi-device" in m.error(), "a multi-device context"
    blob = pack_v3(*nc.ordinary(8, 8, 1, 1), np.full((1, 1), 2), np.full((1, 1), 1), total=4, passes=2, n_a=1, n_b=1)
    assert pc.load_rc(m, blob) == RT_ERR_ARG, "a version-3 load on a multi-device context"
    m.close()


# ------------------------------------------------------------------ 7: the Python front end
def case_python(hostsim: bool):
    """RenderKernel.progress_advance_adaptive / progress_tile_counts agree with the C ABI."""
    import rt_amd
    from conftest import parsed_scene
    P = parsed_scene("cornell")
    img = rt_amd.Image(W, H)
    rk = rt_amd.RenderKernel(W, H, TOTAL, NB, img, P.triangles, P.materials, P.emissive_triangle_indices, P.material_indices,
                             None, rt_amd.BVH(P.triangles), rt_amd.Image.from_rgb(sc.rt_cases.sky("S")), None, device=0,
                             hostsim=hostsim)
    cam = sc.camera_of("cornell")
    rk.set_camera(rt_amd.Camera(cam[:16].reshape(4, 4), float(cam[16])))
    s = pc.session(hostsim, "cornell")
    run = adaptive_run(s)
    rk.progress_begin()
    rk.progress_track_noise()
    rk.progress_advance(2)
    rk.progress_advance(2)
    infos = []
    while True:
        infos.append(rk.progress_advance_adaptive(2, run["T"]))
        assert set(infos[-1]) == set(INFO_KEYS)
        if infos[-1]["active_tiles"] == 0:
            break
    assert infos == run["infos"], "RenderKernel.progress_advance_adaptive vs the C ABI"
    n, na = rk.progress_tile_counts()
    wn, wna = counts(s)
    assert n.dtype == np.int32 and n.shape == (4, 5) and (n == wn).all() and (na == wna).all()
    assert_bits(rk.progress_resolve().pixels, pc.resolve(s), "RenderKernel.progress_resolve of an adaptive progression")
    assert rk.progress_save() == pc.save(s)
    try:
        rk.progress_advance(1)
        raise AssertionError("a uniform advance after the counts diverged did not raise")
    except rt_amd.RtError as e:
        assert "adaptive" in str(e)
    rk.progress_end()
    s.close()
