"""What the post-render stages' GPU tests share: a stream of their own (Stream), a forced kernel that is given back
(forced_variant) and the chain from a tracked progression to the displayed frame around a test's own stages
(post_chain)."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

import meter_cases
import noise_cases as nc
import progress_cases as pc
import rt_amd

vp = ctypes.c_void_p


class Stream:
    """A non-blocking HIP stream and buffers that wait for it alone."""

    def __init__(self):
        from hip_mem import hip
        self.hip = hip()
        self.hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
        self.hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        s = ctypes.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0  # hipStreamNonBlocking
        self.ptr = s.value

    def upload(self, a):
        from hip_mem import DeviceBuffer
        a = np.ascontiguousarray(a)
        b = DeviceBuffer(a.nbytes)
        b.upload(a)  # (a blocking copy: done when it returns)
        return b

    def download(self, b, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert self.hip.hipStreamSynchronize(self.ptr) == 0
        assert self.hip.hipMemcpy(out.ctypes.data, b.ptr, out.nbytes, 2) == 0
        return out

    def close(self):
        if self.ptr:
            self.hip.hipStreamDestroy(self.ptr)
            self.ptr = None


@contextlib.contextmanager
def forced_variant(ctx_fn, key=None, v=0, **more):
    """rt_test_schedule(key, v), and every key of `more`, on the GPU context ctx_fn(False) gives; each key, a variant or
    another schedule key whose default is 0 (mt_blocks), is back at 0 on the way out. For the two-kernel stages 1 is the
    direct kernel and 2 the LDS one."""
    L, h = ctx_fn(False)
    keys = dict(more, **({key: v} if key else {}))

    def put(values):
        for k, x in values.items():
            rt_amd.check(L, L.rt_test_schedule(h, k.encode(), float(x)), h, "rt_test_schedule")
    put(keys)
    try:
        yield
    finally:
        put(dict.fromkeys(keys, 0))


class Chain:
    """The buffers of a post_chain by name, the session they belong to and the stream its device forms run on."""

    def __init__(self, s, stream, w, h):
        self.s, self.L, self.ctx, self.w, self.h = s, s.L, s.ctx, w, h
        self.q = vp(stream) if stream else None
        self.bufs, self.shapes, self.values = {}, {}, {}

    def new(self, name, shape, fill=-3.0, dtype=np.float32):
        """A buffer of the chain, full of `fill`; its pointer."""
        self.bufs[name] = self.s.array(np.full(shape, fill, dtype))
        self.shapes[name] = shape
        return vp(self.bufs[name].ptr)

    def f4(self, name, w=None, h=None):
        return self.new(name, (h or self.h, w or self.w, 4))

    def f1(self, name, w=None, h=None):
        return self.new(name, (h or self.h, w or self.w))

    def p(self, name):
        return vp(self.bufs[name].ptr)

    def get(self, name):
        return self.bufs[name].get()  # (the download waits for the device)

    def call(self, fn, *args):
        """L.fn(ctx, *args, stream), checked."""
        self.s.ok(getattr(self.L, fn)(self.ctx, *args, self.q), fn)


def post_chain(hostsim: bool, stream, stages=(), *, size=None, sigma=False, features=False, bloom=False, display=True):
    """Cornell under the Cornell camera, device forms on one stream:
      the prefix  a tracked [2, 2] progression at `size` (40 x 30), the linear resolve ("linear"), with sigma the noise
                  figure ("sigma"), with features rt_render_features ("albedo", "normal_depth")
      the middle  stage(chain, frame) for each of `stages`, where frame names the buffer that holds the frame so far; a
                  stage that makes a new frame returns its name
      the suffix  with bloom rt_bloom ("bloomed", "layer"; bloom(chain, frame) gives the parameters, True the
                  defaults), with display the histogram ("histogram"), the solve at the defaults (values["exposure"])
                  and rt_display with that exposure to 8 bits ("out8")
    Every buffer by name as it is at the end, and the chain's values."""
    w, h = size or (pc.W, pc.H)
    s = pc.session(hostsim, "cornell")
    pc.begin(s, total=4, w=w, h=h)
    nc.track(s)
    pc.advance(s, 2)
    pc.advance(s, 2)
    C = Chain(s, stream, w, h)
    C.call("rt_progress_resolve_linear_device", C.f4("linear"))
    if sigma:
        C.call("rt_progress_noise_sigma_device", C.f1("sigma"))
    if features:
        C.call("rt_render_features_device", w, h, C.f4("albedo"), C.f4("normal_depth"))
    frame = "linear"
    for stage in stages:
        frame = stage(C, frame) or frame
    fh, fw = C.shapes[frame][:2]
    if bloom:
        p = None if bloom is True else bloom(C, frame)
        C.call("rt_bloom_device", fw, fh, C.p(frame), ctypes.byref(p) if p else None, C.f4("bloomed", fw, fh), C.f4("layer", fw, fh))
        frame = "bloomed"
    if display:
        C.call("rt_meter_device", fw, fh, C.p(frame), C.new("histogram", meter_cases.WORDS, 0xDEADBEEF, np.uint32))
        r = rt_amd.meter_solve(C.get("histogram"), hostsim=hostsim)
        C.values["exposure"] = r["exposure"]
        d = rt_amd.DisplayParams(r["exposure"], 2.2, 0)
        C.call("rt_display_device", fw, fh, C.p(frame), ctypes.byref(d), None, C.new("out8", (fh, fw, 4), 0, np.uint8))
    got = {name: b.get() for name, b in C.bufs.items()}
    got.update(C.values)
    s.close()
    return got


def both_chains(chain):
    """chain(hostsim, stream) on the hostsim build and on the GPU on a stream of its own: (want, got)."""
    want = chain(True, None)
    st = Stream()
    try:
        return want, chain(False, st.ptr)
    finally:
        st.close()
