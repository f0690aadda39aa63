"""What the prior-density tests share (CPU and GPU): the golden cases of tests/golden/prior_density.npz, the host build of
csrc/rvll_prior_density.h (tests/native/hostdensity.hip), the project's parity bound, and sets of priors that mix every kind."""
import ctypes as C
import json
import shutil
import subprocess
from pathlib import Path

import numpy as np

from evidence_amd import _abi, priors as P

HERE = Path(__file__).resolve().parent
GOLDEN = HERE / "golden"
SRC = HERE / "native" / "hostdensity.hip"
LIB = HERE / "native" / "libhostdensity.so"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
dp = C.POINTER(C.c_double)
PARITY = 1e-10                              # the project's parity standard: |delta| <= 1e-10 max(1, |value|)


def golden_cases():
    """[(name, args, x, the reference's logpdf at x, the reference's ppf-against-pdf error)] in the generator's order."""
    z = np.load(GOLDEN / "prior_density.npz")
    cases = json.loads((GOLDEN / "prior_density.json").read_text())["cases"]
    return [(c["name"], tuple(c["args"]), z[f"x{i}"], z[f"v{i}"], c["consistency"]) for i, c in enumerate(cases)]


def case_id(case):
    return f"{case[0]}{tuple(case[1])}"


def assert_parity(got, want, what=""):
    """-inf and NaN in the same places, and the rest within PARITY."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, "-inf differs")
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN differs")
    assert not np.any(got == np.inf) and not np.any(want == np.inf), what
    f = np.isfinite(want)
    err = np.abs(got[f] - want[f]) / np.maximum(1.0, np.abs(want[f]))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= PARITY, (what, worst)
    return worst


def host_lib():
    """The host build of tests/native/hostdensity.hip (the flags of tests/test_hostmath.py), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    csrc = HERE.parent / "evidence_amd" / "csrc"
    deps = [SRC, csrc / "rvll_prior_density.h", HERE.parent / "include" / "rvll.h"]
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950", f"-I{csrc}",
                        f"-I{HERE.parent / 'include'}", str(SRC), "-o", str(LIB)], check=True)
    return C.CDLL(str(LIB))


def host_logpdf(lib, spec, x):
    """prior_logpdf of the host build for a stand-alone spec at x [n]."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    kind, args = int(spec.density[0]), spec.density[1:]
    a = (C.c_double * _abi.DENSITY_NARGS)(*args)
    assert lib.hd_args_ok(C.c_int(kind), a) == 1, spec
    lib.hd_logpdf(C.c_int(kind), a, x.ctypes.data_as(dp), C.c_long(x.size), out.ctypes.data_as(dp))
    return out


# one spec of every stand-alone kind; most supports hold (0, 1) and (0.5, 30), where rows() puts most values
CATALOGUE = [
    P.Uniform(-3.5, 20.0), P.Jeffreys(0.01, 2000.0), P.ModJeffreys(1.0, 999.0), P.UniformFrequency(0.05, 500.0), P.Normal(0.5, 4.0),
    P.LogNormal(0.5, 0.0, 2.0), P.Log10Normal(0.5, 0.7), P.TruncatedRayleigh(3.0, 40.0), P.TruncatedUNormal(0.0, 1.0, -1.0, 25.0),
    P.PowerLaw(-2.0, 0.01, 100.0), P.DoublePowerLaw(-1.5, -3.0, 5.0, 0.01, 100.0), P.Sine(0.0, 180.0), P.Binormal(0.0, 1.0, 5.0, 2.0, 0.3),
    P.AsymmetricNormal(0.0, 1.0, 3.0), P.Alpha(2.0), P.Beta(0.867, 3.03), P.Gamma(2.0, 3.0), P.Uniform(0.0, 10.0),
]
SORTED_DIMS = {0: ((1, 3, 5), "SortedUniform"), 1: ((2, 4), "SortedLogUniform"), 2: ((0,), "SortedUniform")}


def mixed_sets(n_sets, ndim):
    """n_sets lists of ndim entries that walk through CATALOGUE, with None (RVLL_DENSITY_SKIP) at every fifth entry and, where
    ndim allows, a sorted group of 3 (set 0, 4, ...), of 2 (set 1, 5, ...) or of 1 member (set 2, 6, ...)."""
    sets = []
    for a in range(n_sets):
        specs = [None if (a * ndim + d) % 5 == 4 else CATALOGUE[(a * 7 + d) % len(CATALOGUE)] for d in range(ndim)]
        dims, name = SORTED_DIMS.get(a % 4, ((), None))
        if dims and dims[-1] < ndim:
            for d in dims:
                specs[d] = P.SortedUniform(0.0, 1.0) if name == "SortedUniform" else P.SortedLogUniform(0.1, 40.0)
        sets.append(specs)
    return sets


def rows(B, ndim, seed=0):
    """B rows of ndim values: half in (0, 1), a third in (0.5, 30), the rest normal about 0 with width 5 (outside many
    supports); in half of the rows the columns of the sorted groups rise; a few NaN and exact support ends."""
    rng = np.random.default_rng(seed)
    pick = rng.random((B, ndim))
    th = np.where(pick < 0.5, rng.uniform(0.01, 0.99, (B, ndim)),
                  np.where(pick < 0.85, rng.uniform(0.5, 30.0, (B, ndim)), rng.normal(0.0, 5.0, (B, ndim))))
    for dims in ((1, 3, 5), (2, 4)):
        dims = [d for d in dims if d < ndim]
        if len(dims) > 1:
            inorder = np.sort(rng.uniform(0.15, 0.95, (B, len(dims))), axis=1)
            use = rng.random(B) < 0.5
            th[np.ix_(use, dims)] = inorder[use]
    flat = th.reshape(-1)
    where = rng.choice(flat.size, flat.size // 50, replace=False)
    flat[where] = rng.choice([np.nan, 0.0, 1.0, 10.0, 20.0, -3.5, 180.0], where.size)
    return th
