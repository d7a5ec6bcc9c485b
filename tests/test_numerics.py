"""Host-side numerics checks of the arithmetic identities the kernel relies
on (the same checks run on gfx950 in test_gpu_parity.py)."""
from __future__ import annotations

import numpy as np


def division_cases(n: int, seed: int = 1):
    """(a, den) float32 pairs: random magnitudes over the whole exponent
    range, slab-like values, exact quotients, denormals, near-overflow."""
    rng = np.random.default_rng(seed)
    k = n // 4
    a1 = (rng.standard_normal(k) * 2.0 ** rng.integers(-140, 120, k)).astype(np.float32)
    d1 = (rng.standard_normal(k) * 2.0 ** rng.integers(-140, 120, k)).astype(np.float32)
    a2 = rng.uniform(-50, 50, k).astype(np.float32)                     # (d_near - numer)
    d2 = rng.uniform(-1, 1, k).astype(np.float32)                       # n . dir
    m = rng.integers(1, 2 ** 24, k).astype(np.float32)
    d3 = rng.integers(1, 2 ** 12, k).astype(np.float32)
    a3 = (m * d3).astype(np.float32)                                    # exact quotients
    bits = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    a4 = bits.view(np.float32)
    d4 = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32).view(np.float32)
    special_a = np.array([0.0, -0.0, 1.0, 1e-45, 3e38, -3e38, 1e-38, 7.0, 1.0, 2.0], np.float32)
    special_d = np.array([1.0, 3.0, 1e-45, 1e-45, 1e-3, 7e-3, 3.0, 1.5e-45, -3e38, 3.4e38], np.float32)
    a = np.concatenate([a1, a2, a3, a4, special_a])
    d = np.concatenate([d1, d2, d3, d4, special_d])
    ok = np.isfinite(a) & np.isfinite(d) & (d != 0)
    return np.ascontiguousarray(a[ok]), np.ascontiguousarray(d[ok])


def test_slab_division_identity_host():
    """float(double(a) * (1/double(d))) is the correctly rounded a/d for
    finite floats (rt_trace.h slab_div); numpy's float32 divide is IEEE."""
    a, d = division_cases(2_000_000)
    with np.errstate(all="ignore"):
        got = (a.astype(np.float64) * (1.0 / d.astype(np.float64))).astype(np.float32)
        want = a / d
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (a[~same][:4], d[~same][:4], got[~same][:4], want[~same][:4])


REPO = __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__)))


def _native(name):
    import os
    p = os.path.join(REPO, "build", name)
    if not os.path.exists(p):
        import subprocess
        subprocess.run(["make", "-C", REPO, f"build/{name}"], check=True, capture_output=True)
    return p


def test_cdf_fence_search_matches_reference_loop():
    """The counting env-CDF search (rt_trace.h fence_count) returns the
    reference's binary-search result (render_kernel.cpp:532-567) on flat runs,
    ties, out-of-range, +-inf and NaN values, and the host refuses fence
    tables for NaN / decreasing CDFs (tests/native/cdf_check.cpp)."""
    import subprocess
    r = subprocess.run([_native("cdf_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout


def test_libm_restatement_sampled():
    """rt_libm.h against this host's glibc 2.35 on every 4099th float input
    (the exhaustive run is tests/native/libm_check.cpp with stride 1)."""
    import subprocess
    r = subprocess.run([_native("libm_check"), "4099"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------ the libm digests (rt_digest.h)
import pytest  # noqa: E402

import libm_cases as lc  # noqa: E402


def test_libm_digest_fixture_layout():
    """tests/golden/libm_digests.npz holds libm_check's sweep table and one uint64[1024] per sweep."""
    f = lc.fixture()
    table = lc.tool_table()
    assert [t[0] for t in table] == lc.sweep_names()
    assert [t[1] for t in table] == f["fn"].tolist() and [t[2] for t in table] == f["param"].tolist()
    assert [t[3] for t in table] == f["stride"].tolist()
    for name in lc.sweep_names():
        assert f[name].dtype == np.uint64 and f[name].shape == (lc.BLOCKS,)
    assert {0x3f800000 >> 22, 0x42b00000 >> 22, 0x7f800000 >> 22, 0, 0x80000000 >> 22} <= set(lc.CPU_BLOCKS)
    # 8 one-argument rows, 8 + 12 of powf (the fixed exponents' reciprocals are float divisions), 18 + 18 of atan2f
    assert len(table) == 64
    one = np.float32(1.0)
    assert f["param"][8:16].tolist() == [int(np.float32(v).view(np.uint32)) for v in
                                         (5.0, one / np.float32(2.2), one / np.float32(2.4), one / np.float32(1.8), 1.0, 0.5, 2.0, 3.0)]


@pytest.mark.parametrize("name", lc.sweep_names())
def test_libm_digest_blocks_match_fixture(name):
    """This machine's glibc and the host build of rt_libm.h both give the fixture's words on CPU_BLOCKS: the
    fixture is what glibc returns, the tool's digest is the fixture's, and the restatement still matches."""
    want = lc.sweep(name)[3][list(lc.CPU_BLOCKS)]
    glibc, mine = lc.tool_digest_blocks(name, lc.CPU_BLOCKS)
    assert np.array_equal(glibc, want), (name, "glibc", [hex(int(v)) for v in glibc], [hex(int(v)) for v in want])
    assert np.array_equal(mine, want), (name, "rt_libm.h", [hex(int(v)) for v in mine], [hex(int(v)) for v in want])


def test_libm_digest_self_check(tmp_path):
    """The digest notices what it must: one flipped result bit and two swapped results change the word, NaN
    payloads do not, the sign of zero does; rt_digest.h (through libm_check) and numpy agree on the word."""
    rng = np.random.default_rng(22)
    first = 0x3f7ffe00
    v = rng.integers(0, 1 << 32, 1024, dtype=np.uint64).astype(np.uint32)
    v[(v & 0x7fffffff) > 0x7f800000] = 0x3f800000  # (no NaN yet)
    v[7], v[8] = 0x00000000, 0x7f800000

    def word(bits):
        w = lc.tool_digest_values(bits.view(np.float32), first, tmp_path)
        assert w == lc.np_digest(bits.view(np.float32), first), "rt_digest.h vs numpy"
        return w

    base = word(v)
    for k, bit in ((0, 0), (500, 31), (1023, 12)):
        f = v.copy()
        f[k] ^= np.uint32(1 << bit)
        assert word(f) != base, f"a flipped bit {bit} of result {k}"
    s = v.copy()
    s[[100, 101]] = s[[101, 100]]
    assert v[100] != v[101] and word(s) != base, "two swapped results"
    z = v.copy()
    z[7] = 0x80000000
    assert word(z) != base, "-0.0 for 0.0"
    nans = []
    for payload in (0x7fc00000, 0x7f800001, 0xffc00000, 0xffffffff, 0x7fa55555):
        n = v.copy()
        n[9] = payload
        nans.append(word(n))
    assert len(set(nans)) == 1 and nans[0] != base, "every NaN is one NaN, and not the number it replaced"
    inf = v.copy()
    inf[9] = 0x7f800000
    assert word(inf) != nans[0], "inf is no NaN"
    assert lc.tool_digest_values(v.view(np.float32), first + 1, tmp_path) != base, "the same results one index on"
    # and a block's word is the sum over its indices: the sqrtf sweep's block of 1.0, from numpy's IEEE sqrt
    b = 0x3f800000 >> lc.BLOCK_BITS
    with np.errstate(invalid="ignore"):
        assert lc.np_digest(np.sqrt(lc.block_arguments(b, 1)), b << lc.BLOCK_BITS) == int(lc.sweep("sqrtf")[3][b])


def test_libm_check_eval_mode(tmp_path):
    """libm_check --eval returns glibc's results in the sweep's argument order."""
    m = lc.glibc()
    x = np.array([0.3, -2.5, 88.0, 1e-40, np.inf, -0.0, 7.0], np.float32)
    for name, f in (("expf", lambda a: m.expf(a)), ("sincosf.c", lambda a: m.cosf(a)),
                    ("powf.y0", lambda a: m.powf(a, 5.0)), ("powf.x5", lambda a: m.powf(-2.0, a)),
                    ("atan2f.y4", lambda a: m.atan2f(0.5, a)), ("atan2f.x4", lambda a: m.atan2f(a, 0.5))):
        got = lc.glibc_eval(name, x, tmp_path)
        want = np.array([f(float(a)) for a in x], np.float32)
        assert np.array_equal(lc.np_canon(got), lc.np_canon(want)), name
