"""The libm digests (sycl-ray-tracing_amd/csrc/rt_digest.h): tests/golden/libm_digests.npz holds, for every
sweep of tests/native/libm_check.cpp's table, glibc's digest word of each of the 1024 blocks of 2^22 float bit
patterns (tools/gen_golden_libm.py). Shared by tests/test_numerics.py (the host build of rt_libm.h and this
machine's glibc against some blocks) and tests/test_gpu_libm.py (the gfx950 build against all of them).

Helpers only: no tests here."""
from __future__ import annotations

import os
import subprocess

import numpy as np

import golden_io as gio

GOLDEN = os.path.join(gio.GOLDEN, "libm_digests.npz")
BLOCK_BITS = 22
BLOCKS = 1 << (32 - BLOCK_BITS)

# rtdigest::Fn
(FN_EXPF, FN_SINF, FN_COSF, FN_ACOSF, FN_ASINF, FN_SQRTF, FN_SINCOSF_S, FN_SINCOSF_C, FN_POWF_Y, FN_POWF_X, FN_ATAN2F_Y,
 FN_ATAN2F_X) = range(12)

# The blocks the CPU test re-derives for every sweep: those of 0x00000000, 0x3f800000 (1), 0x42b00000 (88: expf's
# abstop 0x42b), 0x4d000000 (2^27: reduce_large), 0x7f800000 (inf and the first NaNs), 0x80000000 (-0),
# 0xc2cff1b4 (-103.97: expf's may_uflowf band) and 0xffffffff (the last negative NaNs).
CPU_BLOCKS = (0x00000000 >> 22, 0x3f800000 >> 22, 0x42b00000 >> 22, 0x4d000000 >> 22, 0x7f800000 >> 22, 0x80000000 >> 22,
              0xc2cff1b4 >> 22, 0xffffffff >> 22)

_fixture = None


def fixture() -> dict:
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        _fixture = {k: z[k] for k in z.files}
    return _fixture


def sweep_names() -> list:
    return [str(n) for n in fixture()["sweeps"]]


def sweep(name: str):
    """(function code, fixed argument's bits, stride, glibc's uint64[1024]) of a sweep."""
    f = fixture()
    k = sweep_names().index(name)
    return int(f["fn"][k]), int(f["param"][k]), int(f["stride"][k]), f[name]


def tool() -> str:
    p = os.path.join(gio.REPO, "build", "libm_check")
    if not os.path.exists(p):
        subprocess.run(["make", "-C", gio.REPO, "build/libm_check"], check=True, capture_output=True)
    return p


def tool_table() -> list:
    """[(name, function code, fixed argument's bits, stride)] of libm_check --list."""
    out = subprocess.run([tool(), "--list"], check=True, capture_output=True, text=True).stdout
    return [(n, int(f), int(p, 16), int(s)) for n, f, p, s in (line.split() for line in out.splitlines())]


def tool_digest_blocks(name: str, blocks):
    """(glibc's words, the host rt_libm's words) of the named blocks, from libm_check --digest-blocks."""
    out = subprocess.run([tool(), "--digest-blocks", name, ",".join(str(b) for b in blocks)], check=True, capture_output=True,
                         text=True, timeout=120).stdout
    rows = [line.split() for line in out.splitlines()]
    assert [int(r[0]) for r in rows] == list(blocks)
    return np.array([int(r[1], 16) for r in rows], np.uint64), np.array([int(r[2], 16) for r in rows], np.uint64)


def tool_digest_values(values, first: int, tmp_path) -> int:
    """libm_check --digest-values: the sum of the terms of `values` taken as f(first), f(first + 1), ..."""
    p = os.path.join(str(tmp_path), "values.bin")
    np.ascontiguousarray(values, np.float32).tofile(p)
    out = subprocess.run([tool(), "--digest-values", p, str(first)], check=True, capture_output=True, text=True).stdout
    return int(out.split()[0], 16)


def glibc_eval(name: str, swept, tmp_path) -> np.ndarray:
    """glibc's results of sweep `name` at the swept float32 arguments, from libm_check --eval."""
    a, b = os.path.join(str(tmp_path), "args.bin"), os.path.join(str(tmp_path), "results.bin")
    np.ascontiguousarray(swept, np.float32).tofile(a)
    subprocess.run([tool(), "--eval", name, a, b], check=True, capture_output=True, timeout=120)
    return np.fromfile(b, np.float32)


def glibc():
    """This machine's libm through ctypes, float in and float out (as tests/test_gpu_parity.py's _glibc)."""
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    for n in ("expf", "sinf", "cosf", "acosf", "asinf"):
        getattr(m, n).restype = ctypes.c_float
        getattr(m, n).argtypes = [ctypes.c_float]
    for n in ("powf", "atan2f"):
        getattr(m, n).restype = ctypes.c_float
        getattr(m, n).argtypes = [ctypes.c_float, ctypes.c_float]
    return m


# ------------------------------------------------------------------ the digest in numpy (a second implementation)
def np_canon(r) -> np.ndarray:
    u = np.ascontiguousarray(r, np.float32).view(np.uint32).copy()
    u[(u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = 0x7fc00000
    return u


def np_digest(values, first: int) -> int:
    """The sum (mod 2^64) of mix((canon(v[k]) << 32) | (first + k))."""
    u = np_canon(values).astype(np.uint64)
    i = (np.uint64(first) + np.arange(u.size, dtype=np.uint64)) & np.uint64(0xffffffff)
    v = (u << np.uint64(32)) | i
    with np.errstate(over="ignore"):
        v = v * np.uint64(0x9E3779B97F4A7C15)
        v ^= v >> np.uint64(29)
        v = v * np.uint64(0xBF58476D1CE4E5B9)
        v ^= v >> np.uint64(32)
        return int(v.sum(dtype=np.uint64))


# ------------------------------------------------------------------ a failing block, element by element (GPU)
def block_arguments(block: int, stride: int) -> np.ndarray:
    """The float32 arguments of a block's summed indices."""
    return np.arange(block << BLOCK_BITS, (block + 1) << BLOCK_BITS, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)


def device_values(name: str, swept) -> np.ndarray:
    """The gfx950 build's results of sweep `name` at the swept arguments, through k_libm (rt_device_libm)."""
    from rt_amd import _capi
    fn, param, _, _ = sweep(name)
    x = np.ascontiguousarray(swept, np.float32)
    fixed = np.full(x.shape, param, np.uint32).view(np.float32)
    code, a, b = {FN_EXPF: (0, x, None), FN_SINF: (2, x, None), FN_COSF: (3, x, None), FN_ACOSF: (4, x, None),
                  FN_ASINF: (5, x, None), FN_SQRTF: (7, x, None), FN_SINCOSF_S: (11, x, None), FN_SINCOSF_C: (12, x, None),
                  FN_POWF_Y: (1, x, fixed), FN_POWF_X: (1, fixed, x), FN_ATAN2F_Y: (6, fixed, x),
                  FN_ATAN2F_X: (6, x, fixed)}[fn]
    out = np.zeros_like(x)
    assert _capi.lib().rt_device_libm(0, code, _capi.ptr(a), _capi.ptr(b), _capi.ptr(out), x.shape[0]) == 0
    return out


def first_difference(name: str, block: int, tmp_path):
    """None, or (argument bits, device result bits, glibc result bits) of the block's first argument at which the
    device and glibc differ (NaN equal to NaN)."""
    _, _, stride, _ = sweep(name)
    x = block_arguments(block, stride)
    got, want = device_values(name, x), glibc_eval(name, x, tmp_path)
    bad = np.flatnonzero(np_canon(got) != np_canon(want))
    if not bad.size:
        return None
    k = int(bad[0])
    return int(x.view(np.uint32)[k]), int(got.view(np.uint32)[k]), int(want.view(np.uint32)[k])
