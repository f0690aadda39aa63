"""Inputs and the host build shared by the tests of the one-division log-L item (rvll_math.h: ItemPool, pool_add, pool_chi2):
tests/test_item_pool_host.py (against mpmath and the oracle) and tests/test_gpu_item_pool.py."""
import ctypes as C
import functools
import shutil
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "hostitem.hip"
LIB = HERE / "native" / "libhostitem.so"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
U = 2.0 ** -53                            # half a unit in the last place of 1: the relative error of one fp64 rounding


def host_lib():
    """The host build of tests/native/hostitem.hip (same flags as tests/test_hostmath.py's), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    hdrs = list((HERE.parent / "evidence_amd" / "csrc").glob("*.h"))
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in [SRC] + hdrs):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{HERE.parent / 'evidence_amd' / 'csrc'}", str(SRC), "-o", str(LIB)], check=True)
    return C.CDLL(str(LIB))


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def pool(lib, num, den, R, var):
    """(res^2 / (2 var), N, D) of the rows of num, den [n, np] through pool_add in planet order and pool_chi2."""
    num, den, R, var = _d(num), _d(den), _d(R), _d(var)
    n, npl = num.shape
    out, nd = np.empty(n), np.empty(2 * n)
    lib.hi_pool(num.ctypes.data_as(dp), den.ctypes.data_as(dp), C.c_long(n), C.c_int(npl), R.ctypes.data_as(dp), var.ctypes.data_as(dp),
                out.ctypes.data_as(dp), nd.ctypes.data_as(dp))
    return out, nd[0::2].copy(), nd[1::2].copy()


def separate(lib, num, den, R, var):
    """The same with one corrected quotient per planet and one for the item: the arithmetic before the pool."""
    num, den, R, var = _d(num), _d(den), _d(R), _d(var)
    n, npl = num.shape
    out = np.empty(n)
    lib.hi_separate(num.ctypes.data_as(dp), den.ctypes.data_as(dp), C.c_long(n), C.c_int(npl), R.ctypes.data_as(dp),
                    var.ctypes.data_as(dp), out.ctypes.data_as(dp))
    return out


def host_loglike(lib, w, theta, tol=1e-4, itmax=10000):
    """log-L of the rows of theta for a workload in the plain parametrisation (evidence_amd.synthetic: k1, period, ecc, omega,
    ma0 free, the epoch fixed; offset and jitter per instrument; no drift) through hi_loglike."""
    names, table = w.parnames, w.table
    npl = sum(1 for nm in names if nm.endswith("_k1"))
    col = lambda nm: theta[:, names.index(nm)]                                  # noqa: E731
    per_planet = lambda suf: _d(np.stack([col(f"planet{p}_{suf}") for p in range(1, npl + 1)], axis=1))   # noqa: E731
    K, Pd, ecc, om, ma0 = (per_planet(s) for s in ("k1", "period", "ecc", "omega", "ma0"))
    epoch = _d(np.tile([w.fixedpardict[f"planet{p}_epoch"] for p in range(1, npl + 1)], (theta.shape[0], 1)))
    off = _d(np.stack([col(f"{nm}_offset") for nm in table.insts], axis=1))
    jit2 = _d(np.stack([col(f"{nm}_jitter") for nm in table.insts], axis=1) ** 2)
    t, y, s2 = _d(table.time), _d(table.vrad), _d(table.svrad * table.svrad)
    inst = np.ascontiguousarray(table.inst_id, dtype=np.int32)
    out = np.empty(theta.shape[0])
    cte = -0.5 * t.size * np.log(2 * np.pi)
    lib.hi_loglike(*(a.ctypes.data_as(dp) for a in (K, Pd, ecc, om, ma0, epoch, off, jit2)), C.c_long(theta.shape[0]), C.c_int(npl),
                   C.c_int(len(table.insts)), t.ctypes.data_as(dp), y.ctypes.data_as(dp), s2.ctypes.data_as(dp),
                   inst.ctypes.data_as(ip), C.c_int(t.size), C.c_double(tol), C.c_int(itmax), C.c_double(cte), out.ctypes.data_as(dp))
    return out


@functools.lru_cache(maxsize=None)
def quotient_rows(npl, n=4000):
    """(num, den, R, var) [n, npl] / [n]: denominators 1 - e cos E over their whole range [0.01, 1.99]; numerators up to a few
    hundred of either sign.  The first quarter of the rows has every denominator at 0.01 (e = 0.99 at periastron in every planet
    at once); the second has numerators of alternating sign that cancel in the sum to 1e-10 of a term, and R within 1e-9 of the
    sum (a perfect fit: the whole cancellation happens in the item's one FMA); the third a planet with nu = 0 (den = 1) in
    position row mod npl."""
    rng = np.random.default_rng(600 + npl)
    den = rng.uniform(0.01, 1.99, (n, npl))
    num = rng.uniform(-300.0, 300.0, (n, npl))
    q = n // 4
    den[:q] = 0.01
    if npl > 1:
        num[q:2 * q, 1::2] = -np.abs(num[q:2 * q, 1::2])
        num[q:2 * q, 0::2] = np.abs(num[q:2 * q, 0::2])
        rest = (num[q:2 * q, 1:] / den[q:2 * q, 1:]).sum(axis=1)
        num[q:2 * q, 0] = (-rest * (1 + 1e-10)) * den[q:2 * q, 0]
    rows = np.arange(2 * q, 3 * q)
    den[rows, rows % npl] = 1.0
    R = rng.uniform(-50.0, 50.0, n)
    R[q:2 * q] = (num[q:2 * q] / den[q:2 * q]).sum(axis=1) * (1 + rng.uniform(-1e-9, 1e-9, q))
    var = rng.uniform(0.25, 2500.0, n)
    for a in (num, den, R, var):
        a.setflags(write=False)
    return num, den, R, var


def exact(num, den, R, var):
    """(sum_p num / den, res^2 / (2 var), |R| + sum_p |num / den|) of every row, from the doubles as they are, to 50 digits."""
    import mpmath
    S, chi, mag = [], [], []
    with mpmath.workdps(50):
        for nr, dr, r, v in zip(num.tolist(), den.tolist(), R.tolist(), var.tolist()):
            qs = [mpmath.mpf(a) / mpmath.mpf(b) for a, b in zip(nr, dr)]
            s = mpmath.fsum(qs)
            res = mpmath.mpf(r) - s
            S.append(s)
            chi.append(res * res / (2 * mpmath.mpf(v)))
            mag.append(abs(mpmath.mpf(r)) + mpmath.fsum([abs(x) for x in qs]))
    return S, chi, mag
