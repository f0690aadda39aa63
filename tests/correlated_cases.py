"""What the correlated-noise tests share (CPU and GPU): epoch tables with interleaved instruments, exact ties, a 3000-day gap and
times near JD 55000, the noise terms with their parameters, the project's parity bound, the host build of
csrc/rvll_celerite.h (tests/native/hostcelerite.hip), the dense definition in long double (dense_reference), and the generators
of rows whose forms differ from lane to lane (mixed_rows), that span a prior's decades (wide_rows) and that sit in the band around
Q = 1/2 (band_rows), with the tables in time order, in decreasing time, all at one time and at a 30-second cadence."""
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


# ---- a reference that is not the limit ----------------------------------------------------------------------------------------------
LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    f"np.longdouble has eps {np.finfo(LD).eps} on this platform: dense_reference needs the 64-bit mantissa of the x87 extended format "
    "to stand above a float64 recursion, and would be no better than log_likelihood_dense here")
_LD_LN_2PI = np.log(8 * np.arctan(LD(1)))


def dense_reference(res, var, t, columns):
    """log_likelihood_dense in np.longdouble, rows at a time: res, var [rows, Ne] (or [Ne]), t [Ne], columns [rows, J, 5] (or
    [J, 5] for every row) the float64 columns as the kernel has them.  The kernel matrix, its Cholesky factor column by column,
    the forward solve and the log-determinant, all vectorised over the rows.  -> longdouble [rows] (a scalar for one row), NaN
    where a column or a residual is not finite or a pivot is not > 0."""
    one = np.ndim(res) == 1
    r = np.atleast_2d(np.asarray(res, dtype=np.float64)).astype(LD)
    v = np.atleast_2d(np.asarray(var, dtype=np.float64)).astype(LD)
    rows, ne = r.shape
    cols = np.asarray(columns, dtype=np.float64)
    cols = np.broadcast_to(cols if cols.ndim == 3 else cols[None], (rows,) + cols.shape[-2:])
    tl = np.asarray(t, dtype=np.float64).astype(LD)
    x = np.abs(tl[:, None] - tl[None, :])
    bad = ~np.isfinite(r).all(axis=1) | ~np.isfinite(cols).all(axis=(1, 2))
    A = np.zeros((rows, ne, ne), dtype=LD)
    A[:, np.arange(ne), np.arange(ne)] = v
    J = cols.shape[1]
    taken = np.zeros((rows, J), dtype=bool)                  # the second column of a pair, summed with the first
    for j in range(J):
        a, b, c, d = (cols[:, j, k].astype(LD)[:, None, None] for k in range(4))
        form = cols[:, j, 4]
        real = (form == correlated.FORM_REAL) & ~bad & ~taken[:, j]
        cosf = (form == correlated.FORM_COS) & ~bad
        if j + 1 < J:
            # the two columns of an SHO below 1/2 (the second is the only real column with a < 0) are +-amp / (2 f) near 1/2 and
            # cancel to amp: a0 exp(-c0 x) + a1 exp(-c1 x) = exp(-c0 x) ((a0 + a1) + a1 expm1(-(c1 - c0) x)), the same function of
            # the same float64 columns with both differences exact, keeps the long double's digits (against mpmath: 2e-15 without)
            pair = real & (cols[:, j + 1, 4] == correlated.FORM_REAL) & (cols[:, j + 1, 0] < 0)
            if pair.any():
                a1, c1 = (cols[pair, j + 1, k].astype(LD)[:, None, None] for k in (0, 2))
                A[pair] += np.exp(-c[pair] * x) * ((a[pair] + a1) + a1 * np.expm1(-(c1 - c[pair]) * x))
                taken[pair, j + 1] = True
                real &= ~pair
        if real.any():
            A[real] += a[real] * np.exp(-c[real] * x)
        if cosf.any():
            A[cosf] += np.exp(-c[cosf] * x) * (a[cosf] * np.cos(d[cosf] * x) + b[cosf] * np.sin(d[cosf] * x))
    L = np.zeros_like(A)
    z = np.zeros((rows, ne), dtype=LD)
    lndet = np.zeros(rows, dtype=LD)
    with np.errstate(all="ignore"):
        for k in range(ne):
            piv = A[:, k, k] - (L[:, k, :k] ** 2).sum(axis=1)
            bad |= ~(piv > 0)
            lkk = np.sqrt(piv)
            L[:, k, k] = lkk
            L[:, k + 1:, k] = (A[:, k + 1:, k] - (L[:, k + 1:, :k] * L[:, None, k, :k]).sum(axis=2)) / lkk[:, None]
            z[:, k] = (r[:, k] - (L[:, k, :k] * z[:, :k]).sum(axis=1)) / lkk
            lndet += np.log(lkk)
        out = -(z * z).sum(axis=1) / 2 - lndet - ne * _LD_LN_2PI / 2
    out[bad] = np.nan
    return out[0] if one else out


def ref_err(got, want):
    """|got - want| / max(1, |want|) against a long-double reference, as float64."""
    want = np.asarray(want, dtype=LD)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want) / np.maximum(1, np.abs(want))).astype(np.float64)


# ---- case generators ---------------------------------------------------------------------------------------------------------------
# every ordered way to fill at most 4 columns from real (1 column) and sho (2 columns), and rotation; term k has prefix gp<k + 1>
COMPOSITIONS = {cid: tuple("real" if ch == "1" else "sho" for ch in cid)
                for cid in ("1", "2", "11", "12", "21", "111", "22", "112", "121", "211", "1111")}
COMPOSITIONS["rotation"] = ("rotation",)
# the sides of Q = 1/2 an SHO cycles through row by row: None draws below (0.01 to 0.45) or above (0.55 to 1e4).  The second SHO
# of a composition cycles through the longer list: 7 and 9 are coprime, so 63 consecutive rows hold every pair of entries.
Q_SIDES = ("below", 0.5 - 1e-6, 0.5 - 1e-9, 0.5, 0.5 + 1e-9, 0.5 + 1e-6, "above")
Q_SIDES_2 = Q_SIDES + ("below", "above")
INVALID_EVERY = 13


def composition_terms(composition):
    return [(kind, f"gp{k + 1}") for k, kind in enumerate(COMPOSITIONS[composition])]


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _split_sigma(rng, total, nterms):
    """Per-term sigmas whose squares sum to total² (row by row)."""
    w = rng.uniform(0.2, 1.0, (nterms, total.shape[0]))
    return total * np.sqrt(w / w.sum(axis=0))


def mixed_rows(composition, n, seed, svmin=1.0):
    """n rows of a composition in which neighbouring rows differ in form: (terms, {name: [n]}).  Every row has its own sigma
    (summed sigma² <= (3 svmin)²) and timescales (2 to 200 days); every SHO's Q cycles through Q_SIDES (the second SHO's through
    Q_SIDES_2); every INVALID_EVERY-th row is invalid in one parameter of one term, rotating through Q = 0, Q < 0, rho = 0,
    tau = inf, sigma = NaN and, for rotation, q0 = 0 and q0 = -0.25."""
    rng = np.random.default_rng([seed, 1])
    terms = composition_terms(composition)
    sig = _split_sigma(rng, rng.uniform(0.5, 3.0, n) * svmin, len(terms))
    rows = np.arange(n)
    values, nsho = {}, 0
    for k, (kind, prefix) in enumerate(terms):
        values[f"{prefix}_sigma"] = sig[k]
        if kind == "real":
            values[f"{prefix}_tau"] = _loguniform(rng, 2.0, 200.0, n)
        elif kind == "sho":
            sides = Q_SIDES_2 if nsho else Q_SIDES
            nsho += 1
            below, above = rng.uniform(0.01, 0.45, n), _loguniform(rng, 0.55, 1e4, n)
            q = np.empty(n)
            for i in rows:
                s = sides[i % len(sides)]
                q[i] = below[i] if s == "below" else above[i] if s == "above" else s
            values[f"{prefix}_rho"] = _loguniform(rng, 2.0, 200.0, n)
            values[f"{prefix}_q"] = q
        else:
            values[f"{prefix}_prot"] = _loguniform(rng, 2.0, 200.0, n)
            values[f"{prefix}_q0"] = _loguniform(rng, 0.05, 5.0, n)
            values[f"{prefix}_dq"] = _loguniform(rng, 0.01, 5.0, n)
            values[f"{prefix}_mix"] = _loguniform(rng, 1e-3, 10.0, n)
    faults = []
    for kind, prefix in terms:
        faults.append((f"{prefix}_sigma", np.nan))
        if kind == "real":
            faults.append((f"{prefix}_tau", np.inf))
        elif kind == "sho":
            faults += [(f"{prefix}_q", 0.0), (f"{prefix}_q", -0.3), (f"{prefix}_rho", 0.0)]
        else:
            faults += [(f"{prefix}_q0", 0.0), (f"{prefix}_q0", -0.25)]
    for m, i in enumerate(range(INVALID_EVERY - 1, n, INVALID_EVERY)):
        name, v = faults[m % len(faults)]
        values[name][i] = v
    return terms, values


def wide_rows(composition, n, seed, svmin=1.0):
    """n rows drawn log-uniformly over a prior's decades: timescales in [0.01, 1e4] days, Q in [0.01, 1e4] but at least 1e-3 from
    1/2, q0 and dq in [1e-3, 1e3], mix in [1e-3, 10], the summed sigma² in [(0.03 svmin)², (30 svmin)²]."""
    rng = np.random.default_rng([seed, 2])
    terms = composition_terms(composition)
    sig = _split_sigma(rng, _loguniform(rng, 0.03, 30.0, n) * svmin, len(terms))
    values = {}
    for k, (kind, prefix) in enumerate(terms):
        values[f"{prefix}_sigma"] = sig[k]
        if kind == "real":
            values[f"{prefix}_tau"] = _loguniform(rng, 0.01, 1e4, n)
        elif kind == "sho":
            q = _loguniform(rng, 0.01, 1e4, n)
            near = np.abs(q - 0.5) < 1e-3
            q[near] = np.where(q[near] < 0.5, 0.5 - 1e-3, 0.5 + 1e-3)
            values[f"{prefix}_rho"] = _loguniform(rng, 0.01, 1e4, n)
            values[f"{prefix}_q"] = q
        else:
            values[f"{prefix}_prot"] = _loguniform(rng, 0.01, 1e4, n)
            values[f"{prefix}_q0"] = _loguniform(rng, 1e-3, 1e3, n)
            values[f"{prefix}_dq"] = _loguniform(rng, 1e-3, 1e3, n)
            values[f"{prefix}_mix"] = _loguniform(rng, 1e-3, 10.0, n)
    return terms, values


BAND_RATIOS = (3.0, 10.0, 30.0, 100.0)
BAND_DQ = (0.0, 1e-9, -1e-9, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4)
BAND_RHO = (0.3, 25.0, 2000.0)


def band_rows(svmin=1.0):
    """The band around Q = 1/2 in which the two columns of an SHO nearly cancel, as a grid of sigma / svmin, Q - 1/2 and rho:
    {"sho": (terms, values)} for an SHO alone, {"rotation": ...} for a rotation term at q0 = 1, dq = 1e-6 (both oscillators far
    from 1/2, 1e-6 apart) and at dq = 1 with q0 = 1e-9 .. 1e-4, which puts its faster oscillator at 1/2 + q0 (q0 <= 0 is
    invalid: there is no side below)."""
    g = np.array([(s, dq, rho) for s in BAND_RATIOS for dq in BAND_DQ for rho in BAND_RHO])
    sho = ([("sho", "gp1")], {"gp1_sigma": g[:, 0] * svmin, "gp1_rho": g[:, 2].copy(), "gp1_q": 0.5 + g[:, 1]})
    r = np.array([(s, q0, dq, prot) for s in BAND_RATIOS for q0, dq in ((1.0, 1e-6), (1e-9, 1.0), (1e-6, 1.0), (1e-5, 1.0), (1e-4, 1.0))
                  for prot in BAND_RHO])
    rot = ([("rotation", "gp1")], {"gp1_sigma": r[:, 0] * svmin, "gp1_prot": r[:, 3].copy(), "gp1_q0": r[:, 1].copy(),
                                   "gp1_dq": r[:, 2].copy(), "gp1_mix": np.full(r.shape[0], 0.5)})
    return {"sho": sho, "rotation": rot}


def row_values(values, i):
    return {name: float(v[i]) for name, v in values.items()}


def rows_columns(terms, values):
    """The definition's columns of every row [n, J, 5] and which rows have a valid covariance: term_columns gave neither None
    nor NaN columns.  The invalid rows' columns are NaN."""
    n = len(next(iter(values.values())))
    J = sum(correlated.RANK[kind] for kind, _ in terms)
    cols, valid = np.full((n, J, 5), np.nan), np.zeros(n, dtype=bool)
    for i in range(n):
        row = []
        for kind, prefix in terms:
            tc = correlated.term_columns(kind, [values[f"{prefix}_{s}"][i] for s in correlated.KINDS[kind][1]])
            if tc is None:
                break
            row += tc
        else:
            cols[i] = row
            valid[i] = np.isfinite(cols[i]).all()
    return cols, valid


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def _one_instrument(time, seed):
    rng = np.random.default_rng(seed)
    ne = len(time)
    return EpochTable.from_arrays(["a"], time, rng.normal(0.0, 4.0, ne), rng.uniform(1.0, 2.0, ne), np.zeros(ne, dtype=np.int32))


def sorted_table(ne=65):
    """One instrument, already in time order (strictly increasing): `order` is the identity."""
    rng = np.random.default_rng(2000 + ne)
    return _one_instrument(55000.25 + np.cumsum(rng.uniform(0.02, 3.0, ne)), 2001 + ne)


def decreasing_table(ne=65):
    """sorted_table listed in decreasing time."""
    s = sorted_table(ne)
    return EpochTable.from_arrays(["a"], s.time[::-1], s.vrad[::-1], s.svrad[::-1], s.inst_id[::-1])


def ties_table(ne=5):
    """Every epoch at the same time: every gap is 0 and Sigma = diag(var) + sum(a) 1 1^T."""
    return _one_instrument(np.full(ne, 55010.5), 2002 + ne)


def cadence_table(ne=65):
    """One night at a 30-second cadence: every gap is small and P is about 1 everywhere."""
    return _one_instrument(55000.25 + np.arange(ne) * (30.0 / 86400.0), 2003 + ne)


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
