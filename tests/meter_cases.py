"""Exposure metering (rt_meter, rt_meter_solve; include/rt_hip.h). The references are model(), the header
comment's rule restated in numpy (the luminance in float32 in the stated operation order, which is bit-exact with
the library because every object is built without contraction, then the bit rule with integer numpy operations),
and solve_model(), the solve's formulas in numpy float64. Neither calls the library.

Inputs are synthetic, so no scene is bound. A frame of w x h pixels is the first w * h entries of a pixel list,
repeated when the frame is longer than the list:
  noise      seeded; luminances log-uniform over 2^-24 .. 2^14, so `under` and `over` are not zero; every fifth
             alpha is a NaN (alpha is ignored)
  specials   NaN, +inf and -inf in each channel; the largest finite channels; negatives, +0, -0, a negative
             luminance from mixed signs, denormals; then, for every bin b, a pixel whose luminance is exactly the
             bin's lower edge asfloat((b + 856) << 20) and one whose luminance is the float below it
             (edge_pixels: grey where a grey value has that luminance, else an (r, g, g) triple).
             Finite channels whose luminance overflows do not exist: the float weights sum to 1 - 1e-12 and a
             search over the 64 largest floats per channel (2 million triples) finds no infinite luminance; grey
             FLT_MAX has the luminance FLT_MAX. The frame carries those pixels, which land in bin 255 as `over`.
  constant   every pixel (0.25, 0.5, 0.125): one bin
  black      every pixel 0: nothing is counted

Shared by tests/test_meter.py (hostsim) and tests/test_meter_gpu.py (gfx950).
Helpers only: no tests here."""
from __future__ import annotations

import ctypes

import numpy as np

import rt_amd
from rt_amd import ptr

f32, u32 = np.float32, np.uint32
WORDS = 264
COUNTED, UNDER, OVER, NONPOSITIVE, NONFINITE, MAX_BITS, MIN_BITS, RESERVED = range(256, 264)
K0, K1 = 856, 1111
FMAX = float(np.finfo(np.float32).max)
# (1, 1) one live thread; (5, 3) part of one wave; (37, 29) and (130, 67) several blocks with a partial last one;
# (64, 4) one block exactly; (257, 1) one block and one pixel
SHAPES = [(1, 1), (5, 3), (37, 29), (130, 67), (64, 4), (257, 1)]
KINDS = ("noise", "specials", "constant", "black")
W709 = (f32(0.2126), f32(0.7152), f32(0.0722))  # the header's float constants
SEED = 11
SOLVE_RTOL = 2.0 ** -22  # one float rounding of a double computation, 4x for libm's exp2 / log1p
DEFAULTS = dict(low=0.10, high=0.95, key=0.18, min_exposure=2.0 ** -8, max_exposure=2.0 ** 12, tau_up=0.0, tau_down=0.0)


# ------------------------------------------------------------------ the reference (numpy)
def luminance32(rgb):
    """float32 luminance in the library's operation order: three rounded products, then the two sums."""
    r, g, b = (np.asarray(rgb[..., i], f32) for i in range(3))
    with np.errstate(all="ignore"):
        return (W709[0] * r + W709[1] * g) + W709[2] * b


def model(rgba) -> np.ndarray:
    """The 264 words of rt_meter_hist for a [h, w, 4] float32 frame."""
    px = np.ascontiguousarray(rgba, f32).reshape(-1, 4)
    L = luminance32(px)
    bits = L.view(u32)
    finite = np.isfinite(px[:, :3]).all(1) & ((bits & u32(0x7F800000)) != u32(0x7F800000))
    with np.errstate(all="ignore"):
        nonpositive = finite & (L <= 0)
    binned = finite & ~nonpositive
    b = bits[binned]
    k = (b >> u32(20)).astype(np.int64)
    hist = np.zeros(WORDS, np.int64)
    hist[:256] = np.bincount(np.clip(k - K0, 0, 255), minlength=256)
    hist[COUNTED] = binned.sum()
    hist[UNDER] = (k < K0).sum()
    hist[OVER] = (k > K1).sum()
    hist[NONPOSITIVE] = nonpositive.sum()
    hist[NONFINITE] = (~finite).sum()
    hist[MAX_BITS] = b.max(initial=0)
    hist[MIN_BITS] = b.min(initial=0xFFFFFFFF)
    return hist.astype(u32)


def solve_model(hist, prev=0.0, dt=0.0, **params) -> dict:
    """rt_meter_solve in numpy float64; the parameters, prev and dt are floats in the C call, so rounded first."""
    p = {k: float(f32(v)) for k, v in dict(DEFAULTS, **params).items()}
    prev, dt = float(f32(prev)), float(f32(dt))
    c = np.asarray(hist[:256], np.int64).copy()
    n = int(hist[COUNTED])
    lo, hi = int(np.floor(p["low"] * n)), int(np.floor((1.0 - p["high"]) * n))
    if lo + hi >= n:
        lo = hi = 0
    for order, cut in ((range(256), lo), (range(255, -1, -1), hi)):
        for b in order:
            d = min(cut, int(c[b]))
            c[b] -= d
            cut -= d
    N = int(c.sum())
    if N == 0:
        e = prev if prev > 0 else 1.5
        return dict(exposure=e, target=e, log2_mean=0.0, valid=False)
    S = int((c * (2 * np.arange(256) - 319)).sum())
    log2_mean = S / (16.0 * N)
    target = float(np.clip(-np.log1p(-p["key"]) / np.exp2(log2_mean), p["min_exposure"], p["max_exposure"]))
    tau = p["tau_up"] if target > prev else p["tau_down"]
    e = target
    if prev > 0 and tau > 0 and dt >= 0:
        with np.errstate(all="ignore"):
            e = float(np.exp2(np.log2(prev) + (np.log2(target) - np.log2(prev)) * (1.0 - np.exp(-dt / tau))))
    return dict(exposure=e, target=target, log2_mean=log2_mean, valid=True)


# ------------------------------------------------------------------ inputs
def asfloat(bits):
    return np.asarray(bits, u32).view(f32)


_edges = {}


def edge_pixels():
    """(rgb [512, 3] float32, grey_hits): for b = 0 .. 255 a pixel whose float32 luminance has exactly the bits
    (b + 856) << 20 (rows 2 b) and one with those bits minus one (rows 2 b + 1). grey_hits: how many of the 256
    lower edges a grey pixel reaches. The weights do not sum to 1 in float32, so the search walks the grey values a
    few ulps around the target; where none fits it walks (r, g, g) triples, whose r moves the luminance in steps of
    a fifth of an ulp."""
    if _edges:
        return _edges["v"]
    rgb = np.zeros((512, 3), f32)
    grey_hits = 0
    steps = np.arange(-24, 25, dtype=np.int64)
    for b in range(256):
        for below in (0, 1):
            want = ((b + K0) << 20) - below
            g = asfloat((want + steps).astype(u32))
            hit = np.nonzero(luminance32(np.stack([g, g, g], -1)).view(u32) == want)[0]
            if hit.size:
                px = (g[hit[0]],) * 3
                grey_hits += 1 - below
            else:
                r, gg = np.meshgrid(asfloat((want + np.arange(-200, 201)).astype(u32)), g)
                ok = np.argwhere(luminance32(np.stack([r, gg, gg], -1)).view(u32) == want)
                assert ok.size, f"no pixel with the luminance bits {want:#x}"
                px = (r[tuple(ok[0])], gg[tuple(ok[0])], gg[tuple(ok[0])])
            rgb[2 * b + below] = px
    rgb.setflags(write=False)
    _edges["v"] = (rgb, grey_hits)
    return _edges["v"]


def _specials() -> np.ndarray:
    nan, inf, big, den = np.nan, np.inf, 3.0e38, 1.0e-40
    head = [(nan, .5, .5), (.5, nan, .5), (.5, .5, nan), (inf, .5, .5), (.5, inf, .5), (.5, .5, inf), (-inf, .5, .5),
            (.5, -inf, .5), (.5, .5, -inf), (inf, -inf, 1.0),          # not finite in a channel
            (big, big, big), (FMAX, FMAX, FMAX), (FMAX, FMAX, 0.0),     # the largest finite channels: still finite
            (-1.0, -2.0, -0.5), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (1.0, -1.0, 0.0), (-FMAX, -FMAX, -FMAX),  # <= 0
            (den, den, den), (0.0, 1.4e-45, 0.0), (den, 0.0, 0.0),      # denormal luminances
            (1e-8, 1e-8, 1e-8), (1e6, 1e6, 1e6), (0.18, 0.18, 0.18)]    # under, over, an ordinary pixel
    rgb = np.concatenate([np.array(head, f32), edge_pixels()[0]])
    return np.concatenate([rgb, np.linspace(-1, 2, len(rgb), dtype=f32)[:, None]], 1)


def frame(kind: str, w: int, h: int, seed: int = SEED) -> np.ndarray:
    """[h, w, 4] float32."""
    n = w * h
    if kind == "noise":
        rng = np.random.default_rng(seed + 1000 * w + h)
        lum = np.exp2(rng.uniform(-24.0, 14.0, n))
        px = np.empty((n, 4), f32)
        px[:, :3] = (lum[:, None] * rng.uniform(0.5, 1.5, (n, 3))).astype(f32)
        px[:, 3] = rng.random(n).astype(f32)
        px[::5, 3] = np.nan
    elif kind == "specials":
        px = np.resize(_specials(), (n, 4))
    elif kind == "constant":
        px = np.tile(np.array([0.25, 0.5, 0.125, 1.0], f32), (n, 1))
    else:
        assert kind == "black"
        px = np.zeros((n, 4), f32)
    return np.ascontiguousarray(px.reshape(h, w, 4))


# ------------------------------------------------------------------ the calls
_ctx = {}


def ctx(hostsim=True):
    """One bare context per library: the stage needs neither a scene nor a camera."""
    if hostsim not in _ctx:
        L = rt_amd.lib(hostsim)
        hnd = ctypes.c_void_p()
        rt_amd.check(L, L.rt_create(0, ctypes.byref(hnd)), None, "rt_create")
        _ctx[hostsim] = (L, hnd)
    return _ctx[hostsim]


def meter(rgba, hostsim=True, code=False, **over):
    """The 264 words of rt_meter, or its return code. over: replacements for the call's arguments by name (w, h,
    src, out)."""
    L, hnd = ctx(hostsim)
    H, W = rgba.shape[:2]
    a = dict(src=rgba, w=W, h=H, out=np.full(WORDS, 0xABCD1234, u32))  # (garbage: the call clears it)
    a.update(over)
    rc = L.rt_meter(hnd, a["w"], a["h"], ptr(a["src"]), ptr(a["out"]))
    if code:
        return rc
    rt_amd.check(L, rc, hnd, "rt_meter")
    return a["out"]


def solve(hist, prev=0.0, dt=0.0, code=False, **params):
    """rt_meter_solve on the hostsim library: its result as a dict, or the return code."""
    L = rt_amd.lib(True)
    p = rt_amd.MeterParams()
    L.rt_meter_default_params(ctypes.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    r = rt_amd.MeterResult()
    h = np.ascontiguousarray(hist, u32)
    rc = L.rt_meter_solve(ptr(h), ctypes.byref(p), ctypes.c_float(prev), ctypes.c_float(dt), ctypes.byref(r))
    if code:
        return rc
    rt_amd.check(L, rc, None, "rt_meter_solve")
    return dict(exposure=float(r.exposure), target=float(r.target), log2_mean=float(r.log2_mean), valid=bool(r.valid))


def hist_of(bins: dict) -> np.ndarray:
    """A hand-built histogram: {bin: count}, counted filled in."""
    h = np.zeros(WORDS, u32)
    for b, c in bins.items():
        h[b] = c
    h[COUNTED] = h[:256].sum()
    h[MIN_BITS] = 0xFFFFFFFF
    return h


_host_cache = {}


def host_result(kind, w, h):
    """hostsim's histogram for a synthetic case, computed once and shared (read-only)."""
    key = (kind, w, h)
    if key not in _host_cache:
        got = meter(frame(kind, w, h))
        got.setflags(write=False)
        _host_cache[key] = got
    return _host_cache[key]


def assert_words(got, want, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
