"""Inputs and the host build shared by the tests of the rotation between Newton steps (rvll_math.h: rotate_mid,
newton_next_sincos): tests/test_rotate_host.py (against mpmath; old rule against new) and tests/test_gpu_rotate.py."""
import ctypes as C
import functools
import math
import shutil
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "hostrotate.hip"
LIB = HERE / "native" / "libhostrotate.so"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
MID_MAX = 7.85398163397448279e-01         # kRotateMidMax: the double below pi/4
CHAIN = 7                                 # the shortcut loop evaluates eight pairs at the most: seven rotations


def host_lib():
    """The host build of tests/native/hostrotate.hip (same flags as tests/test_hostmath.py's), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    hdrs = list((HERE.parent / "evidence_amd" / "csrc").glob("*.h"))
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in [SRC] + hdrs):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{HERE.parent / 'evidence_amd' / 'csrc'}", str(SRC), "-o", str(LIB)], check=True)
    lib = C.CDLL(str(LIB))
    lib.hr_rotate_mid_max.restype = C.c_double
    return lib


def rotate_mid(lib, E, h):
    """(s, c) of sincos_f64(E) rotated by the columns of h ([n] or [n, nrot]) in turn."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(E.size, -1)
    s, c = np.empty(E.size), np.empty(E.size)
    lib.hr_rotate_mid(E.ctypes.data_as(dp), h.ctypes.data_as(dp), C.c_long(E.size), C.c_int(h.shape[1]), s.ctypes.data_as(dp),
                      c.ctypes.data_as(dp))
    return s, c


def solve(lib, M, ecc, rule, tol=1e-4, itmax=10000):
    M, ecc = np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(ecc, dtype=np.float64)
    steps, E = np.empty(M.size, dtype=np.int32), np.empty(M.size)
    lib.hr_solve(M.ctypes.data_as(dp), ecc.ctypes.data_as(dp), C.c_long(M.size), C.c_int(rule), C.c_double(tol), C.c_int(itmax),
                 steps.ctypes.data_as(ip), E.ctypes.data_as(dp))
    return steps, E


EDGE_H = [0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308, 1e-300, 1e-20, -1e-9, 1e-4, -1e-4,
          2.0 ** -6, -(2.0 ** -6), MID_MAX, -MID_MAX, float(np.nextafter(MID_MAX, 0.0))]


@functools.lru_cache(maxsize=None)
def single_vector(n=100_000):
    """(E, h): E over +-1e4 as the mean anomalies of this path are, h over (0, pi/4] of both signs — uniform, log-uniform down
    to 1e-12, and the end points, h = 0 and denormal h."""
    rng = np.random.default_rng(360)
    E = rng.uniform(-1.0e4, 1.0e4, n)
    h = np.where(rng.random(n) < 0.7, rng.uniform(-MID_MAX, MID_MAX, n), rng.choice([-1.0, 1.0], n) * MID_MAX * 10.0 ** rng.uniform(-12, 0, n))
    h[: len(EDGE_H)] = EDGE_H
    assert np.abs(h).max() <= MID_MAX
    E.setflags(write=False)
    h.setflags(write=False)
    return E, h


@functools.lru_cache(maxsize=None)
def chain_vector(n=100_000):
    """(E, H[n, 7]): seven rotations in a row, every one within the bound; a third of the rows the largest steps allowed."""
    rng = np.random.default_rng(361)
    E = rng.uniform(-1.0e4, 1.0e4, n)
    H = rng.uniform(-MID_MAX, MID_MAX, (n, CHAIN))
    big = rng.random(n) < 1 / 3
    H[big] = np.where(rng.random((int(big.sum()), CHAIN)) < 0.5, -MID_MAX, MID_MAX)
    E.setflags(write=False)
    H.setflags(write=False)
    return E, H


def err_vs_mpmath(E, H, s, c):
    """max |s - sin(E + sum H)|, max |c - cos(E + sum H)|, the sum exact, in units of 2^-53."""
    import mpmath
    H = np.asarray(H).reshape(len(E), -1)
    with mpmath.workprec(120):
        es = ec = mpmath.mpf(0)
        for ev, hv, sv, cv in zip(E.tolist(), H.tolist(), s.tolist(), c.tolist()):
            ct, st = mpmath.cos_sin(mpmath.fsum([ev] + hv, absolute=False))
            es = max(es, abs(st - sv))
            ec = max(ec, abs(ct - cv))
        return float(es * 2 ** 53), float(ec * 2 ** 53)


def half_up(x):
    """x rounded up to the next half unit."""
    return math.ceil(2 * x) / 2


# Measured on the host build against mpmath (profiles/math_primitives.txt), in units of 2^-53: sin, cos
ROTATE_MID_MEASURED = (1.934, 1.886)
ROTATE_MID_CHAIN_MEASURED = (4.897, 5.732)


@functools.lru_cache(maxsize=None)
def solve_sample(n=1_000_000):
    """(M, e): e from cfg3's eccentricity prior, Beta(0.867, 3.03), clamped at 0.99 as the layout does; M uniform over +-1e4."""
    rng = np.random.default_rng(362)
    ecc = np.minimum(rng.beta(0.867, 3.03, n), 0.99)
    M = rng.uniform(-1.0e4, 1.0e4, n)
    M.setflags(write=False)
    ecc.setflags(write=False)
    return M, ecc
