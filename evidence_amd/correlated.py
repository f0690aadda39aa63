"""Correlated noise: the log-likelihood of the RV residuals under a celerite covariance.

The likelihood of GpuRVModel is white: a sum over independent epochs with variance svrad² (+ jitter²).  Here the covariance is
Sigma = diag(var) + K with K[n, m] = sum over terms of k(|t_n - t_m|), `var` what the white likelihood uses, and k one of the
celerite family (Foreman-Mackey, Agol, Ambikasaran & Angus 2017), whose semiseparable structure lets the Cholesky factor of
Sigma be found in O(Ne J²) per parameter vector, J the number of columns:

    kind        parameters (under a prefix gp<digits>)       k(x)
    "real"      _sigma, _tau                                 sigma² exp(-x / tau)                               1 column
    "sho"       _sigma, _rho, _q                             celerite2's SHOTerm: w0 = 2 pi / rho, S0 = sigma² / (w0 q)    2 columns
    "rotation"  _sigma, _prot, _q0, _dq, _mix                celerite2's RotationTerm: two SHOs at prot and prot / 2        4 columns

Every parameter is a free parameter of the model (a name in its parnames, with a prior like any other) or a constant in its
fixedpardict; fixed wins, as in layout.compile_layout.  At most 4 terms and 4 columns in all.

A column is (a, b, c, d, form) with k(x) = exp(-c x)(a cos d x + b sin d x); form 0 is a real column (b = d = 0), forms 1 and 2
are the cosine and sine halves of one complex term, which share (a, b, c, d) and count once in K.  An SHO with q >= 1/2 is one
complex term, below 1/2 two real columns; |q - 1/2| is taken as at least 1e-6 on the side q lies on.

This module holds the definitions in numpy — kernel_matrix, log_likelihood_dense (the definition: a dense Cholesky) and
log_likelihood_recursive (the algorithm of csrc/rvll_celerite.h) — and CorrelatedNoiseModel, which evaluates batches on the
GPU (rvll_celerite_loglike_batch).  The GP those terms define, given the data: predict_dense is the definition
of alpha = Sigma^-1 r and of the conditional mean and variance at the data epochs and at query times, predict_recursive the
sweeps of csrc/rvll_celerite_predict.h in numpy, and CorrelatedNoiseModel.predict_batch / activity_corrected the GPU path
(rvll_celerite_predict_batch).  Parameters that give no valid covariance have log-L = -1e30, the reference's sentinel
(rvmodel:203), and FLAG_NOISE_INVALID.
"""
import math
import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _abi

KINDS = {"real": (_abi.NOISE_REAL, ("sigma", "tau")),
         "sho": (_abi.NOISE_SHO, ("sigma", "rho", "q")),
         "rotation": (_abi.NOISE_ROTATION, ("sigma", "prot", "q0", "dq", "mix"))}
RANK = {"real": 1, "sho": 2, "rotation": 4}
Q_CLAMP = 1.0e-6
INVALID_LOGL = -1.0e30
FORM_REAL, FORM_COS, FORM_SIN = 0, 1, 2
_PREFIX = re.compile(r"gp[0-9]+\Z")
_TWO_PI = 2.0 * np.pi


# ---- names -> slots ----------------------------------------------------------------------------------------------------------
def resolve_terms(terms: Sequence[Tuple[str, str]], parnames: Sequence[str], fixedpardict: Dict[str, float]):
    """[(kind, prefix)] -> [(kind, prefix, [(index, value)] per parameter)]: index >= 0 is a position in sorted(parnames), index
    -1 a constant.  KeyError for a name that is neither free nor fixed, ValueError for an unknown kind, a prefix that is not
    gp<digits>, more than 4 terms or more than 4 columns."""
    names = sorted(parnames)
    index = {n: i for i, n in enumerate(names)}
    out, rank = [], 0
    for kind, prefix in terms:
        if kind not in KINDS:
            raise ValueError(f"unknown noise term kind {kind!r}: one of {sorted(KINDS)}")
        if not isinstance(prefix, str) or not _PREFIX.match(prefix):
            raise ValueError(f"noise term prefix {prefix!r} is not of the form gp<digits>")
        slots = []
        for suffix in KINDS[kind][1]:
            name = f"{prefix}_{suffix}"
            if name in fixedpardict:                # fixed overrides free (layout.compile_layout; rvmodel:178)
                slots.append((-1, float(fixedpardict[name])))
            elif name in index:
                slots.append((index[name], 0.0))
            else:
                raise KeyError(name)
        rank += RANK[kind]
        out.append((kind, prefix, slots))
    if not 1 <= len(out) <= _abi.NOISE_MAX_TERMS:
        raise ValueError(f"1 to {_abi.NOISE_MAX_TERMS} noise terms, got {len(out)}")
    if rank > _abi.NOISE_MAX_RANK:
        raise ValueError(f"the terms have {rank} columns, at most {_abi.NOISE_MAX_RANK}")
    return out


# ---- parameters -> columns (csrc/rvll_celerite.h: cel_column, cel_sho_column; the same operations in the same order) ------------
def _finite(*v):
    return all(math.isfinite(x) for x in v)


def _sho_columns(amp, w0, q):
    """An SHO at w0 with quality q and variance amp = S0 w0 q."""
    if q >= 0.5:
        qc = 0.5 + Q_CLAMP if q - 0.5 < Q_CLAMP else q
        f = math.sqrt((2.0 * qc - 1.0) * (2.0 * qc + 1.0))
        a = amp
        b = a / f
        c = w0 / (2.0 * qc)
        d = c * f
        return [(a, b, c, d, FORM_COS), (a, b, c, d, FORM_SIN)]
    qc = 0.5 - Q_CLAMP if 0.5 - q < Q_CLAMP else q
    f = math.sqrt((1.0 - 2.0 * qc) * (1.0 + 2.0 * qc))
    h, g = 0.5 * amp, w0 / (2.0 * qc)
    return [(h * (1.0 + 1.0 / f), 0.0, g * (1.0 - f), 0.0, FORM_REAL), (h * (1.0 - 1.0 / f), 0.0, g * (1.0 + f), 0.0, FORM_REAL)]


def term_columns(kind: str, params: Sequence[float]):
    """The columns [(a, b, c, d, form)] of one term, or None where its parameters are not valid: not finite, sigma < 0, mix < 0,
    tau, rho, q, prot, q0 + 1/2 or dq not > 0."""
    p = [float(x) for x in params]
    if not _finite(*p):
        return None
    if kind == "real":
        sigma, tau = p
        if not (sigma >= 0.0 and tau > 0.0):
            return None
        return [(sigma * sigma, 0.0, 1.0 / tau, 0.0, FORM_REAL)]
    if kind == "sho":
        sigma, rho, q = p
        if not (sigma >= 0.0 and rho > 0.0 and q > 0.0):
            return None
        w0 = _TWO_PI / rho
        return _sho_columns(sigma * sigma, w0, q)                   # S0 w0 q = sigma²
    if kind == "rotation":
        sigma, prot, q0, dq, mix = p
        if not (sigma >= 0.0 and prot > 0.0 and q0 + 0.5 > 0.0 and dq > 0.0 and mix >= 0.0):
            return None
        amp = sigma * sigma / (1.0 + mix)
        cols = []
        for second in (False, True):
            q = 0.5 + q0 if second else 0.5 + q0 + dq
            under = (2.0 * q - 1.0) * (2.0 * q + 1.0)
            if not under > 0.0:                   # an oscillator at or below 1/2 (q0 <= 0): NaN columns, no valid covariance
                cols += [(math.nan,) * 4 + (FORM_COS,), (math.nan,) * 4 + (FORM_SIN,)]
                continue
            w = (2.0 if second else 1.0) * (2.0 * _TWO_PI) * q / (prot * math.sqrt(under))
            cols += _sho_columns(mix * amp if second else amp, w, q)       # S w q of either oscillator
        return cols
    raise ValueError(f"unknown noise term kind {kind!r}")


def _as_columns(columns):
    cols = np.asarray(columns, dtype=np.float64).reshape(-1, 5)
    if cols.shape[0] > _abi.NOISE_MAX_RANK:
        raise ValueError(f"{cols.shape[0]} columns, at most {_abi.NOISE_MAX_RANK}")
    return cols


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def kernel_matrix(t, columns):
    """The dense K [Ne, Ne] of the columns at times t: K[n, m] = sum exp(-c x)(a cos d x + b sin d x), x = |t_n - t_m|, over the
    real columns and the cosine halves (a complex term counts once)."""
    t = np.asarray(t, dtype=np.float64)
    x = np.abs(t[:, None] - t[None, :])
    K = np.zeros_like(x)
    for a, b, c, d, form in _as_columns(columns):
        if int(form) != FORM_SIN:
            K += np.exp(-c * x) * (a * np.cos(d * x) + b * np.sin(d * x))
    return K


def log_likelihood_dense(res, var, t, columns):
    """The definition: -1/2 z^T z - sum ln L_ii - Ne / 2 ln(2 pi) with L the Cholesky factor of diag(var) + K and L z = res.
    INVALID_LOGL where columns is None or the matrix is not positive definite; an O(Ne³) reference, not a product path."""
    res, var = np.asarray(res, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if columns is None or not np.isfinite(res).all():
        return INVALID_LOGL
    cols = _as_columns(columns)
    if not np.isfinite(cols).all():
        return INVALID_LOGL
    try:
        L = np.linalg.cholesky(np.diag(var) + kernel_matrix(t, cols))
    except np.linalg.LinAlgError:
        return INVALID_LOGL
    z = np.linalg.solve(L, res)
    return float(-0.5 * (z @ z) - np.log(np.diag(L)).sum() - 0.5 * res.shape[0] * math.log(_TWO_PI))


PAIR_F = 0.2                                # kCelPairF of csrc/rvll_celerite.h


def _pairs(cols):
    """The near-degenerate SHO pairs among the columns: [(j, s, g, w, u1, u2)] for the pair in columns j, j + 1.  Near Q = 1/2
    the two columns of an SHO hold +-amp / (2 f) (below 1/2), or a and a / f (above), f = sqrt|4 Q² - 1|, and U S U^T subtracts
    terms 1 / f² times what it leaves.  Such a pair (f < PAIR_F) is carried in the basis phi1 = exp(-g x) cosh w x,
    phi2 = exp(-g x) sinh(w x) / w (s = +1, below 1/2: g = (c0 + c1) / 2, w = (c1 - c0) / 2) or the same with cos and sin
    (s = -1, above: g = c, w = d), in which k(x) = u1 phi1 + u2 phi2 with u1 = a0 + a1 or a, u2 = (a0 - a1) w or b d, all of
    order amp, V = (1, 0), and the propagator over a gap is the 2 x 2 matrix [[m11, s w² m21], [m21, m11]] with
    m11 = phi1(gap), m21 = phi2(gap).  The second column of an SHO below 1/2 is the only real column with a < 0."""
    out = []
    a, b, c, d, form = (cols[:, i] for i in range(5))
    for j in range(cols.shape[0] - 1):
        if form[j] == FORM_REAL and form[j + 1] == FORM_REAL and a[j + 1] < 0.0 and c[j + 1] - c[j] < PAIR_F * (c[j + 1] + c[j]):
            w = 0.5 * (c[j + 1] - c[j])
            out.append((j, 1.0, 0.5 * (c[j + 1] + c[j]), w, a[j] + a[j + 1], (a[j] - a[j + 1]) * w))
        elif form[j] == FORM_COS and form[j + 1] == FORM_SIN and d[j] < PAIR_F * c[j]:
            out.append((j, -1.0, c[j], d[j], a[j], b[j] * d[j]))
    return out


def _pair_propagator(s, g, w, dt):
    """(m11, m21) of a pair over a gap dt."""
    y = w * dt
    if s < 0.0:
        E = math.exp(-(g * dt))
        return E * math.cos(y), E * math.sin(y) / w
    if y < 0.5:                                  # sinh y / y by its series: (exp(y) - exp(-y)) / 2 cancels
        E, y2 = math.exp(-(g * dt)), y * y
        ch = sh = 0.0
        for k in range(7, 0, -1):
            ch = ch * y2 / ((2 * k - 1) * (2 * k)) + 1.0
            sh = sh * y2 / ((2 * k) * (2 * k + 1)) + 1.0
        return E * ch, E * (dt * sh)
    p0, p1 = math.exp(-((g - w) * dt)), math.exp(-((g + w) * dt))
    return 0.5 * (p0 + p1), 0.5 * (p0 - p1) / w


def log_likelihood_recursive(res, var, t, columns):
    """The same number by the recursion of csrc/rvll_celerite.h: the epochs in stable time order, t from the first of them
    (exact ties are legal), and per epoch S <- P (S + D W W^T) P^T, f <- P (f + W z) with P = diag exp(-c dt), D = A - U S U^T,
    W = (V - S U) / D, z = r - U f; log-L = -1/2 sum z² / D - 1/2 sum ln D - Ne / 2 ln(2 pi).  A near-degenerate SHO pair
    (_pairs) has a 2 x 2 block in P and constant U and V.  INVALID_LOGL where a D is not > 0."""
    res, var, t = (np.asarray(v, dtype=np.float64) for v in (res, var, t))
    if columns is None or not np.isfinite(res).all():
        return INVALID_LOGL
    cols = _as_columns(columns)
    J = cols.shape[0]
    a, b, c, d = cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]
    form = cols[:, 4].astype(int)
    suma = a[form != FORM_SIN].sum()
    pairs = _pairs(cols)
    order = np.argsort(t, kind="stable")
    ts = t[order] - t[order[0]]
    S, f, W = np.zeros((J, J)), np.zeros(J), np.zeros(J)
    D = z = chi = lndet = 0.0
    with np.errstate(all="ignore"):
        for n, e in enumerate(order):
            if n > 0:
                dt = ts[n] - ts[n - 1]
                P = np.diag(np.exp(-c * dt))
                for j, s, g, w, _, _ in pairs:
                    m11, m21 = _pair_propagator(s, g, w, dt)
                    P[j:j + 2, j:j + 2] = [[m11, s * w * w * m21], [m21, m11]]
                S = P @ (S + D * np.outer(W, W)) @ P.T
                f = P @ (f + W * z)
            cs, sn = np.cos(d * ts[n]), np.sin(d * ts[n])
            U = np.where(form == FORM_SIN, a * sn - b * cs, np.where(form == FORM_COS, a * cs + b * sn, a))
            V = np.where(form == FORM_SIN, sn, np.where(form == FORM_COS, cs, 1.0))
            for j, _, _, _, u1, u2 in pairs:
                U[j:j + 2], V[j:j + 2] = (u1, u2), (1.0, 0.0)
            SU = S @ U
            D = (var[e] + suma) - U @ SU
            if not D > 0.0:
                return INVALID_LOGL
            W = (V - SU) / D
            z = res[e] - U @ f
            chi += z * z / D
            lndet += math.log(D)
    return float(-0.5 * chi - 0.5 * lndet - 0.5 * res.shape[0] * math.log(_TWO_PI))


# ---- prediction: the conditional mean and variance of the GP given the data ---------------------------------------------
class Prediction(NamedTuple):
    """alpha = Sigma^-1 r, the mean and variance of the latent GP at the data epochs (table order), and at the query times (the
    caller's order; None without query times)."""
    alpha: np.ndarray
    mean_data: np.ndarray
    var_data: np.ndarray
    mean: Optional[np.ndarray]
    var: Optional[np.ndarray]


class GpPrediction(NamedTuple):
    """What CorrelatedNoiseModel.predict_batch returns."""
    residual: np.ndarray
    mean_data: np.ndarray
    var_data: np.ndarray
    mean: Optional[np.ndarray]
    var: Optional[np.ndarray]
    logl: np.ndarray
    flags: np.ndarray


def _kernel_values(x, cols):
    """k(x) of the columns at lags x >= 0 (any shape).  The two columns of an SHO below 1/2 (the second is the only real column
    with a < 0) are +-amp / (2 f) near 1/2 and cancel to amp: they enter as exp(-c0 x) ((a0 + a1) + a1 expm1(-(c1 - c0) x)), the
    same function of the same columns, which keeps the digits kernel_matrix's plain sum loses there."""
    k = np.zeros_like(x)
    J, j = cols.shape[0], 0
    while j < J:
        a, b, c, d, form = cols[j]
        if int(form) == FORM_REAL and j + 1 < J and int(cols[j + 1, 4]) == FORM_REAL and cols[j + 1, 0] < 0.0:
            a1, c1 = cols[j + 1, 0], cols[j + 1, 2]
            k += np.exp(-c * x) * ((a + a1) + a1 * np.expm1(-(c1 - c) * x))
            j += 2
            continue
        if int(form) != FORM_SIN:
            k += np.exp(-c * x) * (a * np.cos(d * x) + b * np.sin(d * x))
        j += 1
    return k


def predict_dense(res, var, t, columns, times=None):
    """The definition: alpha = Sigma^-1 r with Sigma = diag(var) + K, mean(x) = K(x, t) alpha and
    var(x) = k(0) - K(x, t) Sigma^-1 K(t, x), at the data epochs and at `times`.  Every time is taken as its float64 difference
    from the first epoch in time order, as the log-L path takes them.  An O(Ne³) reference, not a product path."""
    res, var, t = (np.asarray(v, dtype=np.float64) for v in (res, var, t))
    cols = _as_columns(columns)
    ts = t - t.min()
    K = _kernel_values(np.abs(ts[:, None] - ts[None, :]), cols)
    Sigma = np.diag(var) + K
    alpha = np.linalg.solve(Sigma, res)
    k0 = _kernel_values(np.zeros(1), cols)[0]
    mean_data = K @ alpha
    var_data = k0 - np.einsum("nm,mn->n", K, np.linalg.solve(Sigma, K))
    if times is None:
        return Prediction(alpha, mean_data, var_data, None, None)
    xs = np.asarray(times, dtype=np.float64).reshape(-1) - t.min()
    Kx = _kernel_values(np.abs(xs[:, None] - ts[None, :]), cols)
    return Prediction(alpha, mean_data, var_data, Kx @ alpha, k0 - np.einsum("xn,nx->x", Kx, np.linalg.solve(Sigma, Kx.T)))


def _generators(cols, pairs, t, dt):
    """U and V at time t (from the first epoch) and the propagator P [J, J] over a gap dt >= 0, in the row's basis: diagonal
    exp(-c dt), with the 2 x 2 block and the constant U = (u1, u2), V = (1, 0) of every prepared pair (_pairs)."""
    a, b, c, d = cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3]
    form = cols[:, 4].astype(int)
    P = np.diag(np.exp(-c * dt))
    cs, sn = np.cos(d * t), np.sin(d * t)
    U = np.where(form == FORM_SIN, a * sn - b * cs, np.where(form == FORM_COS, a * cs + b * sn, a))
    V = np.where(form == FORM_SIN, sn, np.where(form == FORM_COS, cs, 1.0))
    for j, s, g, w, u1, u2 in pairs:
        m11, m21 = _pair_propagator(s, g, w, dt)
        P[j:j + 2, j:j + 2] = [[m11, s * w * w * m21], [m21, m11]]
        U[j:j + 2], V[j:j + 2] = (u1, u2), (1.0, 0.0)
    return U, V, P


def _basis_kernel(cols, pairs, x):
    """k(x) at one lag x >= 0 in the row's basis: u1 phi1(x) + u2 phi2(x) for a prepared pair, whose plain columns cancel."""
    k, taken = 0.0, set()
    for j, s, g, w, u1, u2 in pairs:
        m11, m21 = _pair_propagator(s, g, w, x)
        k += u1 * m11 + u2 * m21
        taken |= {j, j + 1}
    for j, (a, b, c, d, form) in enumerate(cols):
        if j not in taken and int(form) != FORM_SIN:
            k += math.exp(-c * x) * (a * math.cos(d * x) + b * math.sin(d * x))
    return k


def predict_recursive(res, var, t, columns, times=None, mutate=None):
    """predict_dense's numbers in O((Ne + M) J²) (O(M Ne J) for the variance at the query times) by the sweeps of
    csrc/rvll_celerite_predict.h, in the basis log_likelihood_recursive works in:
        forward    the factor: W_n, D_n, z_n of every epoch in time order
        backward   g = 0, M = 0 after the last epoch; alpha_n = z_n / D_n - W_n . g, m = M W_n, Z_nn = 1 / D_n + W_n . m
                   (the diagonal of Sigma^-1), G_n = g + U_n alpha_n, then g <- P_n^T G_n and
                   M <- P_n^T (M + Z_nn U U^T - U m^T - m U^T) P_n; mean_data_n = r_n - var_n alpha_n,
                   var_data_n = var_n - var_n² Z_nn; a query x in [t_(n-1), t_n) takes V(x) . P(t_n - x)^T G_n
        forward    F_n = P_n F_(n-1) + V_n alpha_n; a query x in [t_n, t_(n+1)) adds U(x) . P(x - t_n) F_n
        variance   var(x) = sum a - sum w_n² / D_n with w = L^-1 k(x) by forward substitution through W and D
    Returns None where the factorisation fails (a pivot not > 0).  mutate: a defect to inject, for the tests that show the
    cases can tell ("drop_tie", "transpose", "last_g", "no_forward")."""
    res, var, t = (np.asarray(v, dtype=np.float64) for v in (res, var, t))
    if columns is None or not np.isfinite(res).all():
        return None
    cols = _as_columns(columns)
    if not np.isfinite(cols).all():
        return None
    J, ne = cols.shape[0], t.shape[0]
    form = cols[:, 4].astype(int)
    suma = cols[form != FORM_SIN, 0].sum()
    pairs = _pairs(cols)
    order = np.argsort(t, kind="stable")
    ts = t[order] - t[order[0]]
    dts = np.diff(ts, prepend=ts[0])
    if mutate == "drop_tie":                                     # a tie treated as a gap of a second
        dts = np.where((dts == 0.0) & (np.arange(ne) > 0), 1.0 / 86400.0, dts)
    r, v = res[order], var[order]
    Us, Vs, Ps = np.empty((ne, J)), np.empty((ne, J)), np.empty((ne, J, J))
    Ws, Ds, zs = np.empty((ne, J)), np.empty(ne), np.empty(ne)
    S, f, W = np.zeros((J, J)), np.zeros(J), np.zeros(J)
    D = z = 0.0
    with np.errstate(all="ignore"):
        for n in range(ne):
            U, V, P = _generators(cols, pairs, ts[n], dts[n])
            S = P @ (S + D * np.outer(W, W)) @ P.T
            f = P @ (f + W * z)
            SU = S @ U
            D = (v[n] + suma) - U @ SU
            if not D > 0.0:
                return None
            W = (V - SU) / D
            z = r[n] - U @ f
            Us[n], Vs[n], Ps[n], Ws[n], Ds[n], zs[n] = U, V, P, W, D, z
        if times is None:
            xs = np.empty(0)
        else:
            xs = np.asarray(times, dtype=np.float64).reshape(-1) - t[order[0]]
        qorder = np.argsort(xs, kind="stable")
        n0 = np.searchsorted(ts, xs, side="right") - 1             # the last epoch at or before the query, -1 before the first
        mean = np.zeros(xs.shape[0])
        # backward
        alpha, zdiag = np.empty(ne), np.empty(ne)
        g, M = np.zeros(J), np.zeros((J, J))
        for n in range(ne - 1, -1, -1):
            U, P, W = Us[n], Ps[n], Ws[n]
            if mutate == "transpose" and pairs:
                P = P.T
            alpha[n] = zs[n] / Ds[n] - W @ g
            m = M @ W
            zdiag[n] = 1.0 / Ds[n] + W @ m
            G = g + U * alpha[n]
            for q in qorder[n0[qorder] == n - 1]:
                _, Vx, Px = _generators(cols, pairs, xs[q], ts[n] - xs[q])
                mean[q] = Vx @ (Px.T @ G)
            g = P.T @ (g if (mutate == "last_g" and n == ne - 1) else G)
            M = P.T @ (M + zdiag[n] * np.outer(U, U) - np.outer(U, m) - np.outer(m, U)) @ P
        # forward
        F = np.zeros(J)
        for n in range(ne):
            F = Ps[n] @ F + Vs[n] * alpha[n]
            if mutate == "no_forward":
                continue
            for q in qorder[n0[qorder] == n]:
                Ux, _, Px = _generators(cols, pairs, xs[q], xs[q] - ts[n])
                mean[q] += Ux @ (Px @ F)
        # the variance at the query times
        vq = np.empty(xs.shape[0])
        for q in range(xs.shape[0]):
            f, w, acc = np.zeros(J), 0.0, 0.0
            W = np.zeros(J)
            for n in range(ne):
                f = Ps[n] @ (f + W * w)
                w = _basis_kernel(cols, pairs, abs(xs[q] - ts[n])) - Us[n] @ f
                W = Ws[n]
                acc += w * w / Ds[n]
            vq[q] = suma - acc
    out_alpha, mean_data, var_data = np.empty(ne), np.empty(ne), np.empty(ne)
    out_alpha[order] = alpha
    mean_data[order] = r - v * alpha
    var_data[order] = v - v * v * zdiag
    if times is None:
        return Prediction(out_alpha, mean_data, var_data, None, None)
    return Prediction(out_alpha, mean_data, var_data, mean, vq)


# ---- the GPU path ---------------------------------------------------------------------------------------------------------------------
class CorrelatedNoiseModel:
    """A GpuRVModel's likelihood with celerite noise terms added to its covariance, evaluated on the model's GPU.

    model   a GpuRVModel (precision "fp64") whose parnames / fixedpardict hold the terms' parameters: compile_layout ignores
            names it does not know, so the model itself is unchanged by them and its priordict covers them like any other name
    terms   [(kind, prefix)], e.g. [("sho", "gp1")] for gp1_sigma, gp1_rho, gp1_q

    parnames, ndim, log_likelihood(_batch), prior_transform(_batch) and prior_loglike_batch make it a drop-in for the model in
    callbacks.make_ultranest_callbacks(gp, vectorized=True), callbacks.make_polychord_callbacks(gp) and as
    run_nested_slice(gp.prior_transform_batch, gp.log_likelihood_batch, gp.ndim, prior_loglike=gp.prior_loglike_batch, ...) or
    run_nested_ensemble(gp.prior_transform_batch, gp.log_likelihood_batch, gp.ndim, seeds, walker_runs=gp.slice_walk_runs, ...);
    the results go through merge, posterior, marginals, fip and sensitivity as they are.  predict_batch gives the GP itself for
    finished draws: its mean and variance at the data epochs and at query times; activity_corrected the velocities without it.

    Not offered: the device walks, the resident live sets, region_runs and the scalar server (low_latency=True) evaluate the
    white likelihood inside their kernels; do not pass the model's walker / live / region callables along with this likelihood.
    """

    def __init__(self, model, terms):
        self.model = model
        self.parnames = list(model.parnames)
        self.fixedpardict, self.datadict, self.nplanets, self.table = model.fixedpardict, model.datadict, model.nplanets, model.table
        self.terms = resolve_terms(terms, self.parnames, model.fixedpardict)
        self.rank = sum(RANK[kind] for kind, _, _ in self.terms)
        self.order = np.ascontiguousarray(np.argsort(model.table.time, kind="stable"), dtype=np.int32)
        self._terms_c = (_abi.NoiseTerm * len(self.terms))()
        for i, (kind, _, slots) in enumerate(self.terms):
            self._terms_c[i].kind = KINDS[kind][0]
            for q, (idx, val) in enumerate(slots):
                self._terms_c[i].par[q] = _abi.Slot.free(idx) if idx >= 0 else _abi.Slot.fixed(val)
            for q in range(len(slots), 5):
                self._terms_c[i].par[q] = _abi.Slot.fixed(0.0)

    @property
    def ndim(self):
        return len(self.parnames)

    def _call(self, X, from_cube, timing=None):
        X = self.model._theta2d(X)
        n = X.shape[0]
        out, flags = np.empty(n, dtype=np.float64), np.zeros(n, dtype=np.int32)
        theta = np.empty((n, self.ndim)) if from_cube else None
        ms = np.zeros(2)
        _abi.check(self.model._lib.rvll_celerite_loglike_batch(
            self.model._h, _abi.as_dp(X), n, int(from_cube), self._terms_c, len(self.terms), _abi.as_ip(self.order),
            _abi.as_dp(theta) if from_cube else None, _abi.as_dp(out), _abi.as_ip(flags), _abi.as_dp(ms)))
        if timing is not None:
            timing.update(residuals_ms=float(ms[0]), solve_ms=float(ms[1]))
        return theta, out, flags

    def log_likelihood_batch(self, X, return_flags=False, timing=None):
        """log-L of every row of X [n, ndim] -> float64 [n]; with return_flags also int32 [n] (FLAG_INVALID_ORBIT alone for an
        invalid orbit, FLAG_NOISE_INVALID for noise parameters without a valid covariance; log-L is -1e30 for both).  timing: a
        dict that receives residuals_ms and solve_ms."""
        _, out, flags = self._call(X, False, timing)
        return (out, flags) if return_flags else out

    def predict_batch(self, thetas, times=None, return_var=False, timing=None):
        """The GP given the data, for every row of thetas [n, ndim] (rvll_celerite_predict_batch; the definition is
        predict_dense on the model's residuals): a GpPrediction with residual, mean_data and var_data [n, Ne] in table order, mean
        [n, M] at `times` in the order given (None without times), var [n, M] with return_var (None without: it costs
        O(M Ne J) a row where the rest costs O((Ne + M) J²)), and logl and flags [n], the bits of log_likelihood_batch.  A row
        with a flag is NaN in every array.  timing: a dict that receives residuals_ms, factor_ms, sweeps_ms and variance_ms."""
        X = self.model._theta2d(thetas)
        n, ne = X.shape[0], self.order.shape[0]
        tq = None if times is None else np.ascontiguousarray(np.asarray(times, dtype=np.float64).reshape(-1))
        m = 0 if tq is None else tq.shape[0]
        want_var = bool(return_var) and tq is not None
        residual, mean_data, var_data = (np.empty((n, ne)) for _ in range(3))
        mean = None if tq is None else np.empty((n, m))
        var = np.empty((n, m)) if want_var else None
        logl, flags, ms = np.empty(n), np.zeros(n, dtype=np.int32), np.zeros(4)
        _abi.check(self.model._lib.rvll_celerite_predict_batch(
            self.model._h, _abi.as_dp(X), n, self._terms_c, len(self.terms), _abi.as_ip(self.order),
            _abi.as_dp(tq) if m else None, m, int(want_var), _abi.as_dp(residual), _abi.as_dp(mean_data), _abi.as_dp(var_data),
            _abi.as_dp(mean) if m else None, _abi.as_dp(var) if want_var and m else None, _abi.as_dp(logl), _abi.as_ip(flags),
            _abi.as_dp(ms)))
        if timing is not None:
            timing.update(residuals_ms=float(ms[0]), factor_ms=float(ms[1]), sweeps_ms=float(ms[2]), variance_ms=float(ms[3]))
        return GpPrediction(residual, mean_data, var_data, mean, var, logl, flags)

    def activity_corrected(self, theta):
        """The velocities with the GP's mean at the data epochs taken out, model.table.vrad - mean_data [Ne], for one theta: the
        series to fold or to feed a periodogram.  ValueError where theta has no valid orbit or covariance."""
        theta = np.asarray(theta, dtype=np.float64)
        if theta.size != self.ndim:
            raise ValueError(f"expected {self.ndim} parameters, got {theta.size}")
        p = self.predict_batch(theta.reshape(1, -1))
        if p.flags[0]:
            raise ValueError(f"theta has no prediction (flags {int(p.flags[0])})")
        return np.asarray(self.model.table.vrad, dtype=np.float64) - p.mean_data[0]

    def log_likelihood(self, x):
        x = np.asarray(x, dtype=np.float64)
        if x.size != self.ndim:
            raise ValueError(f"expected {self.ndim} parameters, got {x.size}")
        return float(self.log_likelihood_batch(x.reshape(1, -1))[0])

    def prior_transform_batch(self, cubes):
        return self.model.prior_transform_batch(cubes)

    def prior_transform(self, cube):
        return self.model.prior_transform(cube)

    def prior_loglike_batch(self, cubes, return_flags=False, timing=None):
        """prior(cubes) -> theta -> log-L in one call, theta staying on the device in between: (theta, logl), the bits of
        prior_transform_batch and of log_likelihood_batch on its result."""
        theta, out, flags = self._call(cubes, True, timing)
        return (theta, out, flags) if return_flags else (theta, out)

    def slice_walk_runs(self, cube, theta, logl, run_start, lstar, chol, wrapped=None, nsteps=10, max_rounds=200, seeds=(),
                        proposal=None, step_width=None):
        """walker_runs= of run_nested_ensemble under this likelihood (the model's own slice_walk_runs walks under the white one):
        rows run_start[r] .. run_start[r + 1] are the walkers of run r, which take nsteps chord moves inside logL > lstar[r] with
        the whitening factor chol[r], drawn from default_rng(seeds[r]).  The walk is the host's (nested._host_chord_walk); every
        shrink round of a run is one prior_loglike_batch call.  Returns (cube, theta, logl, ncalls[R])."""
        from .nested import _evaluator, _host_chord_walk
        if proposal not in (None, "chord"):
            raise ValueError("the correlated-noise walk is the chord walk")
        cube = np.array(self.model._theta2d(cube), dtype=np.float64, order="C")
        theta = np.array(self.model._theta2d(theta), dtype=np.float64, order="C")
        logl = np.array(logl, dtype=np.float64).reshape(-1)
        run_start = np.asarray(run_start, dtype=np.int64).reshape(-1)
        nrun = run_start.shape[0] - 1
        if nrun < 0 or run_start[0] != 0 or run_start[-1] != cube.shape[0] or len(lstar) != nrun or len(seeds) != nrun:
            raise ValueError("run_start must rise from 0 to the number of walkers, with one lstar and one seed per run")
        evaluate = _evaluator(None, None, self.prior_loglike_batch)
        wr = None if wrapped is None else np.asarray(wrapped, dtype=bool)
        ncalls = []
        for r in range(nrun):
            rows = slice(int(run_start[r]), int(run_start[r + 1]))
            rng = np.random.default_rng(int(seeds[r]) & (2 ** 64 - 1))
            steps = int(nsteps if np.ndim(nsteps) == 0 else nsteps[r])
            ncalls.append(_host_chord_walk(cube[rows], theta[rows], logl[rows], float(lstar[r]), np.asarray(chol[r], dtype=np.float64),
                                           wr, steps, rng, evaluate))
        return cube, theta, logl, ncalls

    def params(self, theta_row):
        """Per term the values of its parameters for one parameter vector."""
        th = np.asarray(theta_row, dtype=np.float64).ravel()
        return [[th[idx] if idx >= 0 else val for idx, val in slots] for _, _, slots in self.terms]

    def columns(self, theta_row):
        """The definition's columns [J, 5] for one parameter vector, or None where a term's parameters are not valid."""
        cols: List[tuple] = []
        for (kind, _, _), p in zip(self.terms, self.params(theta_row)):
            tc = term_columns(kind, p)
            if tc is None:
                return None
            cols += tc
        return np.asarray(cols, dtype=np.float64)
