"""Records tests/golden/libm_digests.npz: what this machine's glibc returns over every sweep of
tests/native/libm_check.cpp's table (libm_check --list), as the digest of rt_digest.h: one
uint64[1024] per sweep, one word per block of 2^22 consecutive float bit patterns.

libm_check --digest evaluates glibc and the host build of rt_libm.h side by side. Nothing is written
unless the two agree on every block of every sweep: a difference is a bug in rt_libm.h, to be fixed
first. The GPU test (tests/test_gpu_libm.py) holds the gfx950 build of rt_libm.h to these words, the
CPU test (tests/test_numerics.py) re-derives a few blocks of each sweep.

About 1e11 evaluations per evaluator: minutes of CPU. The file is written with fixed zip time stamps, so
a second run on the same glibc gives the same bytes.

  python tools/gen_golden_libm.py [OUT]
"""
import ctypes
import io
import os
import subprocess
import sys
import time
import zipfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "libm_digests.npz")
BLOCKS = 1024


def libm_check() -> str:
    subprocess.run(["make", "-C", REPO, "build/libm_check"], check=True, capture_output=True)
    return os.path.join(REPO, "build", "libm_check")


def sweep_table(tool: str):
    """[(name, function code, fixed argument's bits, stride)] of libm_check --list."""
    out = subprocess.run([tool, "--list"], check=True, capture_output=True, text=True).stdout
    return [(n, int(f), int(p, 16), int(s)) for n, f, p, s in (line.split() for line in out.splitlines())]


def digest_words(tool: str, sweep: str, blocks=None):
    """(blocks, glibc's words, rt_libm's words) of libm_check --digest / --digest-blocks."""
    args = [tool, "--digest", sweep] if blocks is None else [tool, "--digest-blocks", sweep, ",".join(map(str, blocks))]
    out = subprocess.run(args, check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines()]
    return (np.array([int(r[0]) for r in rows], np.int32), np.array([int(r[1], 16) for r in rows], np.uint64),
            np.array([int(r[2], 16) for r in rows], np.uint64))


def glibc_version() -> str:
    f = ctypes.CDLL(None).gnu_get_libc_version
    f.restype = ctypes.c_char_p
    return f().decode()


def write_npz(path: str, arrays: dict) -> None:
    """np.savez_compressed's layout with every member's time stamp fixed."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    tool = libm_check()
    table = sweep_table(tool)
    d = {"glibc": np.array(glibc_version()), "sweeps": np.array([t[0] for t in table]),
         "fn": np.array([t[1] for t in table], np.int32), "param": np.array([t[2] for t in table], np.uint32),
         "stride": np.array([t[3] for t in table], np.int32)}
    bad = 0
    for name, fn, param, stride in table:
        t0 = time.time()
        b, g, m = digest_words(tool, name)
        assert np.array_equal(b, np.arange(BLOCKS))
        diff = np.flatnonzero(g != m)
        print(f"{name:12s} fn {fn:2d} fixed 0x{param:08x} stride {stride}: {time.time() - t0:6.1f} s, "
              f"{diff.size} blocks differ" + (f" (first: {diff[0]})" if diff.size else ""), flush=True)
        bad += diff.size
        d[name] = g
    if bad:
        sys.exit(f"glibc {glibc_version()} and the host build of rt_libm.h differ on {bad} blocks: nothing written")
    write_npz(out, d)
    print("wrote", out, os.path.getsize(out), "bytes; glibc", glibc_version())
