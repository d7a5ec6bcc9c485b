"""The gfx950 build of rt_libm.h against glibc over whole float sweeps, by digest.

tests/golden/libm_digests.npz holds glibc's digest word (rt_digest.h) of every block of 2^22 float bit patterns of
every sweep of tests/native/libm_check.cpp's table: the one-argument functions over all 2^32 inputs, rt_sincosf's two
results, powf over every x at eight exponents and over every fourth y at twelve bases, atan2f over every eighth x at
eighteen y and the other way round. k_libm_digest evaluates the same sweeps on the device and sums the same terms;
one differing result anywhere in a block changes the block's word. On a difference the first differing block is read
back element by element through k_libm, and the first differing argument is reported with glibc's result."""
from __future__ import annotations

import time

import numpy as np
import pytest

import libm_cases as lc

from rt_amd import _capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", lc.sweep_names())
def test_gpu_libm_digest_matches_glibc(name, tmp_path):
    fn, param, stride, want = lc.sweep(name)
    got = np.zeros(lc.BLOCKS, np.uint64)
    t0 = time.perf_counter()
    assert _capi.lib().rt_device_libm_digest(0, fn, param, stride, _capi.ptr(got)) == 0
    print(f"{name}: fn {fn} fixed 0x{param:08x} stride {stride}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    diff = np.flatnonzero(got != want)
    if diff.size:
        block = int(diff[0])
        d = lc.first_difference(name, block, tmp_path)
        where = (f"first differing argument 0x{d[0]:08x}: device 0x{d[1]:08x}, glibc 0x{d[2]:08x}" if d else
                 "k_libm agrees with glibc on every element of it: the digest kernel and k_libm differ")
        pytest.fail(f"{name} (fn {fn}, fixed argument 0x{param:08x}, stride {stride}): {diff.size} of {lc.BLOCKS} blocks "
                    f"differ from glibc {lc.fixture()['glibc']}, the first is block {block}; {where}")


@pytest.mark.parametrize("name", ["sincosf.s", "sincosf.c", "powf.x5", "atan2f.y17"])
def test_gpu_libm_block_readback(name, tmp_path):
    """The path a failing sweep is reported through, on a block that holds 1.0: k_libm's element-wise results
    (rt_sincosf's two, and the two argument orders of powf and atan2f) against libm_check --eval."""
    assert lc.first_difference(name, 0x3f800000 >> lc.BLOCK_BITS, tmp_path) is None


def test_gpu_libm_atanf_readback(tmp_path):
    """k_libm's atanf (atan2f(x, 1)) is the atan2f sweep at fixed x = 1, element by element."""
    name = "atan2f.x2"
    assert lc.sweep(name)[:2] == (lc.FN_ATAN2F_X, 0x3f800000)
    x = lc.block_arguments(0x3ee00000 >> lc.BLOCK_BITS, 1)  # (7/16: the first of atanf's interval ends)
    out = np.zeros_like(x)
    assert _capi.lib().rt_device_libm(0, 13, _capi.ptr(x), None, _capi.ptr(out), x.shape[0]) == 0
    assert np.array_equal(lc.np_canon(out), lc.np_canon(lc.glibc_eval(name, x, tmp_path)))


def test_gpu_libm_digest_arguments():
    L = _capi.lib()
    out = np.zeros(lc.BLOCKS, np.uint64)
    for fn, stride, o in ((-1, 1, out), (12, 1, out), (0, 0, out), (0, 3, out), (0, 512, out), (0, 1, None)):
        assert L.rt_device_libm_digest(0, fn, 0, stride, _capi.ptr(o)) == _capi.RT_ERR_ARG
