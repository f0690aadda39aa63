"""What the correlated-noise tests share (CPU and GPU): epoch tables with interleaved instruments, exact ties, a 3000-day gap and
times near JD 55000, the noise terms with their parameters, the project's parity bound, and the host build of
csrc/rvll_celerite.h (tests/native/hostcelerite.hip)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

from evidence_amd import correlated
from evidence_amd.data import EpochTable

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "hostcelerite.hip"
LIB = HERE / "native" / "libhostcelerite.so"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PARITY = 1e-10                              # the project's parity standard: |delta| <= 1e-10 max(1, |value|)
EPOCH_BLOCK = 32                            # kCelEpochs of csrc/rvll_celerite.hip: the epochs of an LDS tile
NE_CASES = (1, 2, 3, EPOCH_BLOCK - 1, EPOCH_BLOCK, EPOCH_BLOCK + 1, 2 * EPOCH_BLOCK + 1)
INSTS = ["a", "b"]

# (id, [(kind, prefix)], {name: value}); sqrt(var) >= 1 and sigma <= 3 keep sqrt(var) >= sigma / 100
TERM_CASES = [
    ("real", [("real", "gp1")], {"gp1_sigma": 3.0, "gp1_tau": 20.0}),
    ("sho_q0.2", [("sho", "gp1")], {"gp1_sigma": 3.0, "gp1_rho": 25.0, "gp1_q": 0.2}),
    ("sho_q0.5-", [("sho", "gp1")], {"gp1_sigma": 3.0, "gp1_rho": 25.0, "gp1_q": 0.5 - 1e-6}),
    ("sho_q0.5+", [("sho", "gp1")], {"gp1_sigma": 3.0, "gp1_rho": 25.0, "gp1_q": 0.5 + 1e-6}),
    ("sho_q4", [("sho", "gp1")], {"gp1_sigma": 3.0, "gp1_rho": 25.0, "gp1_q": 4.0}),
    ("sho_q300", [("sho", "gp1")], {"gp1_sigma": 3.0, "gp1_rho": 25.0, "gp1_q": 300.0}),
    ("sho+real", [("sho", "gp1"), ("real", "gp2")], {"gp1_sigma": 2.0, "gp1_rho": 11.0, "gp1_q": 2.5, "gp2_sigma": 1.5, "gp2_tau": 60.0}),
    ("rotation", [("rotation", "gp1")], {"gp1_sigma": 3.0, "gp1_prot": 25.0, "gp1_q0": 1.0, "gp1_dq": 0.5, "gp1_mix": 0.5}),
]


def make_table(ne, seed=0):
    """ne epochs of two instruments near JD 55000: nights of up to three epochs, every fifth epoch an exact tie with the one
    before it, one 3000-day gap in the middle; the instruments alternate along time while the table lists instrument a's epochs
    first, so the table is not in time order."""
    rng = np.random.default_rng(1000 + 17 * ne + seed)
    t = np.empty(ne)
    now = 55000.25
    for n in range(ne):
        if n > 0:
            if n % 5 == 4:
                step = 0.0                                   # an exact tie
            elif n % 3 == 0:
                step = float(rng.integers(1, 4)) + rng.uniform(-0.1, 0.1)      # the next night, or a few on
            else:
                step = rng.uniform(0.01, 0.08)               # the same night
            if n == ne // 2:
                step += 3000.0
            now = now + step
        t[n] = now
    inst = np.arange(ne) % 2                                 # along time
    table_order = np.concatenate([np.flatnonzero(inst == 0), np.flatnonzero(inst == 1)])
    time = t[table_order]
    vrad = rng.normal(0.0, 4.0, ne)
    svrad = rng.uniform(1.0, 2.0, ne)
    return EpochTable.from_arrays(INSTS, time, vrad, svrad, inst[table_order])


def case_columns(terms, values):
    """The definition's columns of a case."""
    cols = []
    for kind, prefix in terms:
        cols += correlated.term_columns(kind, [values[f"{prefix}_{s}"] for s in correlated.KINDS[kind][1]])
    return np.asarray(cols)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def host_lib():
    """The host build of tests/native/hostcelerite.hip (the flags of tests/prior_density_cases.py), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    csrc = HERE.parent / "evidence_amd" / "csrc"
    deps = [SRC, csrc / "rvll_celerite.h", csrc / "rvll_math.h", HERE.parent / "include" / "rvll.h"]
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950", f"-I{csrc}",
                        f"-I{HERE.parent / 'include'}", str(SRC), "-o", str(LIB)], check=True)
    return C.CDLL(str(LIB))


def host_loglike(lib, terms, values, res, var, t):
    """(log-L, flag) of the host build for one row: the kernel's own source, fed the epochs in stable time order."""
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    kind, sub, par = [], [], []
    for k, prefix in terms:
        p = [values[f"{prefix}_{s}"] for s in correlated.KINDS[k][1]]
        p += [0.0] * (5 - len(p))
        for s in range(correlated.RANK[k]):
            kind.append(correlated.KINDS[k][0])
            sub.append(s)
            par.append(p)
    J = len(kind)
    order = np.argsort(t, kind="stable")
    ts = np.ascontiguousarray(t[order] - t[order[0]])
    dts = np.ascontiguousarray(np.diff(ts, prepend=ts[0]))
    r, v = np.ascontiguousarray(res[order]), np.ascontiguousarray(var[order])
    kind_c, sub_c = (C.c_int * J)(*kind), (C.c_int * J)(*sub)
    par_c = np.ascontiguousarray(par, dtype=np.float64)
    logl, flag = C.c_double(), C.c_int()
    cte = -0.5 * len(ts) * np.log(2.0 * np.pi)
    rc = lib.hc_loglike(J, kind_c, sub_c, par_c.ctypes.data_as(dp), len(ts), ts.ctypes.data_as(dp), dts.ctypes.data_as(dp),
                        r.ctypes.data_as(dp), v.ctypes.data_as(dp), C.c_double(cte), C.byref(logl), C.byref(flag))
    assert rc == 0
    return logl.value, flag.value
