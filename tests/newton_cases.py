"""Inputs and the host build shared by the tests of the Newton step's fused residuals (rvll_math.h: newton_residuals):
tests/test_newton_fused_host.py (against 50-digit arithmetic; fused against separately rounded) and tests/test_gpu_newton_fused.py."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np

from rotate_cases import HIPCC

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "hostnewton.hip"
LIB = HERE / "native" / "libhostnewton.so"
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
SEPARATE, FUSED = 0, 1


def host_lib():
    """The host build of tests/native/hostnewton.hip (same flags as tests/rotate_cases.py's), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    hdrs = list((HERE.parent / "evidence_amd" / "csrc").glob("*.h"))
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in [SRC] + hdrs):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{HERE.parent / 'evidence_amd' / 'csrc'}", str(SRC), "-o", str(LIB)], check=True)
    return C.CDLL(str(LIB))


def _p(a):
    return a.ctypes.data_as(dp)


def pair(lib, E):
    E = np.ascontiguousarray(E, dtype=np.float64)
    s, c = np.empty(E.size), np.empty(E.size)
    lib.hn_pair(_p(E), C.c_long(E.size), _p(s), _p(c))
    return s, c


def residuals(lib, E, s, c, ecc, M, form):
    """(f, f') of one Newton step in the given form."""
    E, s, c, ecc, M = (np.ascontiguousarray(a, dtype=np.float64) for a in (E, s, c, ecc, M))
    f, fp = np.empty(E.size), np.empty(E.size)
    lib.hn_residuals(_p(E), _p(s), _p(c), _p(ecc), _p(M), C.c_long(E.size), C.c_int(form), _p(f), _p(fp))
    return f, fp


def solve(lib, M, ecc, form, tol=1e-4, itmax=10000):
    """(steps, E, cos nu, sin nu) of the first pass's rule with the residuals in the given form."""
    M, ecc = np.ascontiguousarray(M, dtype=np.float64), np.ascontiguousarray(ecc, dtype=np.float64)
    steps, E, cn, sn = np.empty(M.size, dtype=np.int32), np.empty(M.size), np.empty(M.size), np.empty(M.size)
    lib.hn_solve(_p(M), _p(ecc), C.c_long(M.size), C.c_int(form), C.c_double(tol), C.c_int(itmax), steps.ctypes.data_as(ip), _p(E),
                 _p(cn), _p(sn))
    return steps, E, cn, sn


@functools.lru_cache(maxsize=None)
def residual_rows(n=100_000):
    """(E, s, c, e, M): E over +-1e4 on the first half of the rows and over +-10 on the second, e over [0, 0.99], (s, c) the pair
    the solver holds at E, M = E - e s moved by up to 1e-3 (a step of the iteration near its root, and f = 0 exactly on some)."""
    lib = host_lib()
    rng = np.random.default_rng(370)
    E = np.concatenate([rng.uniform(-1.0e4, 1.0e4, n // 2), rng.uniform(-10.0, 10.0, n - n // 2)])
    ecc = rng.uniform(0.0, 0.99, n)
    ecc[:4] = [0.0, 0.99, 0.5, np.nextafter(0.99, 0)]
    s, c = pair(lib, E)
    M = (E - ecc * s) + rng.uniform(-1.0e-3, 1.0e-3, n) * (rng.random(n) < 0.9)
    for a in (E, s, c, ecc, M):
        a.setflags(write=False)
    return E, s, c, ecc, M


@functools.lru_cache(maxsize=None)
def high_ecc_sample(which, n=1_000_000):
    """(M, e) of the two high-eccentricity samples: e in [0.9, 0.9925] with |M| <= 10, e in [0.95, 0.9925] with |M| <= 100 — the
    eccentricity clamped at 0.99 as the layout does."""
    lo, mmax, seed = ((0.9, 10.0, 371), (0.95, 100.0, 372))[which]
    rng = np.random.default_rng(seed)
    ecc = np.minimum(rng.uniform(lo, 0.9925, n), 0.99)
    M = rng.uniform(-mmax, mmax, n)
    M.setflags(write=False)
    ecc.setflags(write=False)
    return M, ecc


N_EPOCHS, N_POINTS, N_LONG = 70, 192, 48   # 70 epochs: every wave of 64 items holds two points; the last 48 rows: long periods
# Eccentricities: none, the class bounds of the rotation (0.3, 0.6), the eccentricity at which the first step can reach pi/4
# (0.617) and one ulp either side, and high and wandering ones
ECCS = np.array([0.0, 0.3, 0.6, np.nextafter(0.617, 0), 0.617, np.nextafter(0.617, 1), 0.8, 0.9, 0.97])
ECCS_LONG = np.array([0.9, 0.93, 0.95, 0.97, 0.98, 0.99])


def gpu_case(nplanets):
    """(table, parnames, fixed, theta): 2 instruments; planet p of row i at ECCS[(4 i + 3 p) mod 9], so that neighbouring rows —
    the two points of a wave — and the planets of a row differ in class.  The last N_LONG rows have periods of 4000 .. 8000 days
    about an epoch inside the data, |M| <= 10, where the separately rounded and the fused residuals differ most often, with
    planet 1 at e = 0.9 .. 0.99."""
    from test_gpu_loglike import _synthetic_case
    rng = np.random.default_rng(373 + nplanets)
    table, free, fixed, ranges, _ = _synthetic_case(rng, N_EPOCHS, nplanets, 2, False, 0, False)
    theta = np.stack([rng.uniform(*ranges[nm], N_POINTS) for nm in free], axis=1)
    rows = np.arange(N_POINTS)
    for p in range(1, nplanets + 1):
        theta[:, free.index(f"planet{p}_ecc")] = ECCS[(4 * rows + 3 * p) % ECCS.size]
        theta[:, free.index(f"planet{p}_period")] = rng.uniform(2.0, 40.0, N_POINTS)          # many orbits: M covers every phase
        theta[-N_LONG:, free.index(f"planet{p}_period")] = rng.uniform(4000.0, 8000.0, N_LONG)
    theta[-N_LONG:, free.index("planet1_ecc")] = ECCS_LONG[np.arange(N_LONG) % ECCS_LONG.size]
    return table, free, fixed, theta


def reduced_case():
    """(table, parnames, fixed, theta) of the reduced-precision record tests/golden/loglike_reduced_np5.npz: five planets, 64
    epochs, 130 points."""
    from test_gpu_loglike import _synthetic_case
    rng = np.random.default_rng(379)
    table, free, fixed, ranges, _ = _synthetic_case(rng, 64, 5, 2, False, 0, False)
    theta = np.stack([rng.uniform(*ranges[nm], 130) for nm in free], axis=1)
    return table, free, fixed, theta


@functools.lru_cache(maxsize=None)
def residual_records(n=4096):
    """[n, 5] rows (E, s, c, e, M) of residual_rows(), both ranges of E."""
    E, s, c, ecc, M = residual_rows()
    pick = np.concatenate([np.arange(n // 2), E.size // 2 + np.arange(n - n // 2)])
    rec = np.stack([a[pick] for a in (E, s, c, ecc, M)], axis=1)
    rec.setflags(write=False)
    return rec
