"""A minimal batched nested-sampling driver — the seam through which a sampler feeds the GPU.

The reference delegates sampling to PolyChord / UltraNest (third-party, not in the checkout,
not installed here) and only supplies `prior(cube)` and `loglike(theta)`
(evidence/ultranest/__init__.py:165-185).  This driver consumes callbacks with UltraNest's
`vectorized=True` signatures — prior((n, ndim)) -> (n, ndim), loglike((n, ndim)) -> (n,) — and
exists so that BASELINE.json configs[0] (400 live points through the callback boundary) and the
reference's Gaussian known-answer tests (tests/test_polychord.py:75-151: ln Z = -2.0768 in 1-D,
-4.1536 in 2-D) can run end to end.  It is deliberately simple: one bounding ellipsoid in the unit
cube, rejection sampling in batches, one replacement per iteration.  It is not a substitute for
UltraNest's region/step samplers on hard posteriors.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import time

import numpy as np

from .settings import polychord_defaults, ultranest_defaults
from .stepout import check_proposal


@dataclass
class NestedResult:
    logz: float
    logzerr: float
    niter: int
    ncall: int
    information: float
    samples: np.ndarray          # dead + final live points (theta)
    logl: np.ndarray
    logwt: np.ndarray            # log posterior weights (normalised)
    timing: dict = None          # resident live set: seconds in the order step, waiting for the live step, and the loop turns
    nclusters: np.ndarray = None  # clustering=True: the clusters of the survivors, one entry per iteration (None when off)
    nlive: int = None            # the schedule the run died by (shrinkage.replicates reads it): nlive live points,
    kbatch: int = None           # kbatch deaths per iteration (run_nested: 1)
    logl_birth: np.ndarray = None  # per row (the order of logl): the contour it was drawn above — -inf for an initial point, else the
                                   # lstar of the iteration that drew it (the insertion-index test reads it; insertion.py)
    nsteps_trace: np.ndarray = None  # adaptive_nsteps: the step count every iteration walked with (None when off; adapt.py)
    far_fraction: np.ndarray = None  # adaptive_nsteps: the far walkers' share of the counted ones per iteration, NaN where none counted
    nlive_row: np.ndarray = None  # a merged run (merge.py): the live count at every death, which varies from row to row
    run_index: np.ndarray = None  # a merged run: the input run every row comes from
    region_fallbacks: int = None  # proposal="region": the points the chord walk supplied because the region draw stayed short
    region_efficiency: np.ndarray = None  # proposal="region": accepted / likelihood calls of the region draw, per iteration (NaN: no call)
    region_calls: np.ndarray = None  # proposal="region": the region draw's likelihood calls per iteration
    region_fallback_calls: int = None  # proposal="region": the likelihood calls of the fallback walks


def _logaddexp_many(x):
    m = np.max(x)
    return m + np.log(np.sum(np.exp(x - m))) if np.isfinite(m) else m


class _Ellipsoid:
    """Bounding ellipsoid of the live points in the unit cube, enlarged."""

    def __init__(self, u, enlarge):
        self.ndim = u.shape[1]
        self.mean = u.mean(axis=0)
        d = u - self.mean
        cov = d.T @ d / max(1, u.shape[0] - 1) + 1e-12 * np.eye(self.ndim)
        self.chol = np.linalg.cholesky(cov)
        z = np.linalg.solve(self.chol, d.T)
        self.radius = np.sqrt(np.max(np.sum(z * z, axis=0))) * enlarge

    def sample(self, rng, n):
        z = rng.standard_normal((n, self.ndim))
        z *= (rng.random(n) ** (1.0 / self.ndim) / np.linalg.norm(z, axis=1))[:, None]
        return self.mean + self.radius * (z @ self.chol.T)


def run_nested(prior: Callable, loglike: Callable, ndim: int, nlive: Optional[int] = None, dlogz: float = 0.5,
               max_iter: int = 200000, max_calls: int = 5_000_000, batch: int = 1024, enlarge: float = 1.25, update_every: Optional[int] = None,
               seed: int = 0) -> NestedResult:
    """Nested sampling with vectorized callbacks.  Stops when the live points can add less than
    `dlogz` to ln Z (UltraNest's dlogz, evidence/ultranest/__init__.py:182), at `max_iter` replacements,
    or — so that a collapsing acceptance rate can never spin forever — once `max_calls` likelihood
    evaluations have been spent (the result then covers the iterations completed so far)."""
    rng = np.random.default_rng(seed)
    nlive = int(nlive or ultranest_defaults(ndim)["nlive"])          # the reference's default: 25 ndim
    u = rng.random((nlive, ndim))
    theta = np.asarray(prior(u), dtype=np.float64)
    logl = np.asarray(loglike(theta), dtype=np.float64)
    ncall = nlive
    update_every = update_every or max(1, nlive // 5)
    dead_theta, dead_logl, dead_logw = [], [], []
    birth, dead_birth = np.full(nlive, -np.inf), []
    logz, h, logx = -np.inf, 0.0, 0.0
    pool_u = pool_t = pool_l = None
    pos = 0
    it = 0
    while it < max_iter:
        worst = int(np.argmin(logl))
        lmin = logl[worst]
        logx_new = -(it + 1) / nlive
        logw = np.log(np.exp(logx) - np.exp(logx_new)) + lmin          # prior-mass shell x likelihood
        logz_new = np.logaddexp(logz, logw)
        # information H (Skilling 2006), updated incrementally
        h_old_term = np.exp(logz - logz_new) * (h + logz) if np.isfinite(logz) else 0.0
        h = np.exp(logw - logz_new) * lmin + h_old_term - logz_new
        logz, logx = logz_new, logx_new
        dead_theta.append(theta[worst].copy()); dead_logl.append(lmin); dead_logw.append(logw)
        dead_birth.append(birth[worst])
        # replacement: the first pooled candidate above the threshold.  A pool drawn from an older
        # (larger) ellipsoid stays valid — it is uniform on a superset of the constrained region.
        found = False
        while not found:
            if (pool_u is None or pos >= len(pool_u)) and ncall >= max_calls:
                break
            if pool_u is None or pos >= len(pool_u):
                cand = _Ellipsoid(u, enlarge).sample(rng, batch)
                cand = cand[np.all((cand >= 0.0) & (cand < 1.0), axis=1)]
                if len(cand) == 0:
                    continue
                pool_u = cand
                pool_t = np.asarray(prior(pool_u), dtype=np.float64)
                pool_l = np.asarray(loglike(pool_t), dtype=np.float64)      # one batch = one GPU launch
                ncall += len(pool_u)
                pos = 0
            while pos < len(pool_u):
                k = pos
                pos += 1
                if pool_l[k] > lmin:
                    u[worst], theta[worst], logl[worst] = pool_u[k], pool_t[k], pool_l[k]
                    birth[worst] = lmin
                    found = True
                    break
        if not found:                      # budget exhausted: the point removed above stays dead, stop here
            logl[worst] = -np.inf
            keep = np.isfinite(logl)
            u, theta, logl, birth = u[keep], theta[keep], logl[keep], birth[keep]
            it += 1
            break
        it += 1
        if it % update_every == 0:
            pool_u, pos = None, 0                                          # refresh the region now and then
        if np.max(logl) + logx < logz + np.log(np.expm1(dlogz)):           # remaining live mass is negligible
            break
    return _finish(logz, h, logx, it, ncall, nlive, 1, [np.array(dead_theta), theta], [np.array(dead_logl, dtype=np.float64)],
                   [np.array(dead_logw, dtype=np.float64)], logl, [np.array(dead_birth, dtype=np.float64), birth])


# --------------------------------------------------------------------------------------------------
# Batched nested slice sampling: the proposal scheme that keeps a GPU busy.
# --------------------------------------------------------------------------------------------------
def _chord(u, d, wrapped):
    """Range [tmin, tmax] (tmin < 0 < tmax) of t for which u + t d stays inside the unit cube; circular
    parameters have no walls and only limit |t d_i| to half a turn."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (0.0 - u) / d
        t1 = (1.0 - u) / d
    lo = np.where(d != 0, np.minimum(t0, t1), -np.inf)
    hi = np.where(d != 0, np.maximum(t0, t1), np.inf)
    if wrapped is not None and wrapped.any():
        with np.errstate(divide="ignore"):
            half = np.where(d != 0, 0.5 / np.abs(d), np.inf)
        lo = np.where(wrapped, -half, lo)
        hi = np.where(wrapped, half, hi)
    return lo.max(axis=1), hi.min(axis=1)


_POOL = None


def _helper():
    """One helper thread for calls that block on the GPU while the host has arithmetic of its own to do."""
    global _POOL
    if _POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        _POOL = ThreadPoolExecutor(max_workers=1, thread_name_prefix="rvll-live")
    return _POOL


def _stable_argsort(x):
    """np.argsort(x, kind="stable"), by way of the (vectorised, ~8x faster) unstable sort whenever that is provably
    the same permutation: no two equal neighbours in the sorted order means no ties to break."""
    order = np.argsort(x)
    xs = x[order]
    if np.any(xs[1:] == xs[:-1]) or np.isnan(xs[-1] if xs.size else 0.0):
        return np.argsort(x, kind="stable")
    return order


def _deaths(logz, h, logx, dl, nlive, kbatch):
    """The kbatch deaths of an iteration in order, live count nlive - i while they die — vectorised (this loop used to cost
    more than the likelihood calls): X shrinks by exp(-1/(nlive - i)), w_i = (X_{i-1} - X_i) L_i, Z accumulates, and the
    information H follows from A = sum_j w_j ln L_j / Z = H + ln Z.  dl: the dying points' log-L in ascending order.
    Returns (logw, logz, h, logx) after them."""
    logx_seq = logx - np.cumsum(1.0 / (nlive - np.arange(kbatch)))
    logx_prev = np.concatenate([[logx], logx_seq[:-1]])
    logw = logx_prev + np.log1p(-np.exp(logx_seq - logx_prev)) + dl
    logz_seq = np.logaddexp.accumulate(np.concatenate([[logz], logw]))[1:]
    big = max(logz, float(np.max(logw))) if np.isfinite(logz) else float(np.max(logw))
    a_prev = np.exp(logz - big) * (h + logz) if np.isfinite(logz) else 0.0
    a_last = np.exp(big - logz_seq[-1]) * (a_prev + float(np.sum(np.exp(logw - big) * dl)))
    logz, logx = float(logz_seq[-1]), float(logx_seq[-1])
    return logw, logz, float(a_last - logz), logx


def _deaths_runs(logz, h, logx, dl, nlive, kbatch):
    """_deaths for A runs at once — the resident ensemble, whose running runs are all at the same iteration and so share logx
    and the shell widths: logz, h [A], dl [A, kbatch] (each row ascending).  Row a gives the bits _deaths gives for
    (logz[a], h[a], logx, dl[a]): the same elementwise operations in the same order, and row reductions (logaddexp.accumulate,
    sum along the last axis) that follow the 1-D order (tests/test_nested_resident_ensemble_host.py checks it bitwise).
    Returns (logw [A, kbatch], logz [A], h [A], logx)."""
    logx_seq = logx - np.cumsum(1.0 / (nlive - np.arange(kbatch)))
    logx_prev = np.concatenate([[logx], logx_seq[:-1]])
    logw = logx_prev + np.log1p(-np.exp(logx_seq - logx_prev)) + dl
    logz_seq = np.logaddexp.accumulate(np.concatenate([logz[:, None], logw], axis=1), axis=1)[:, 1:]
    fin = np.isfinite(logz)
    top = np.max(logw, axis=1)
    big = np.where(fin & ~(top > logz), logz, top)                 # max(logz, top) as Python's max picks it; top alone at -inf
    with np.errstate(invalid="ignore"):
        a_prev = np.where(fin, np.exp(logz - big) * (h + logz), 0.0)
    logz_new = logz_seq[:, -1].copy()
    a_last = np.exp(big - logz_new) * (a_prev + np.sum(np.exp(logw - big[:, None]) * dl, axis=1))
    return logw, logz_new, a_last - logz_new, float(logx_seq[-1])


def _covariance(ua):
    d0 = ua - ua.mean(axis=0)
    return d0.T @ d0 / max(1, len(ua) - 1) + 1e-14 * np.eye(ua.shape[1])


def _whitening(ua):
    """Lower-triangular factor of the covariance of the unit-cube rows ua (the surviving live points)."""
    return np.linalg.cholesky(_covariance(ua))


# ---- clustering of the survivors (clustering=True) ---------------------------------------------------------
_M64 = 2 ** 64 - 1
_BOOT_MUL = 0x9E3779B97F4A7C15          # bootstrap seed of an iteration: seed * _BOOT_MUL + it
_GROUP_MUL = 0xD1B54A32D192ED03         # walk seed of cluster c > 0: walk_seed + c * _GROUP_MUL


def _cluster_scale(ua):
    """The clustering metric of the survivors ua: 1 / the per-dimension spread of their covariance (as _whitening forms it)."""
    return 1.0 / np.sqrt(np.diag(_covariance(ua)))


def _cluster_factors(ua, labels, ncl, chol):
    """The whitening factor of every cluster: its own where it has at least 2 ndim rows, the run's global one otherwise."""
    if ncl <= 1:
        return [chol]
    need = 2 * ua.shape[1]
    return [_whitening(ua[labels == c]) if np.count_nonzero(labels == c) >= need else chol for c in range(ncl)]


def _walk_groups(cw, factors, walk_seed):
    """The walkers grouped by the cluster of their start row (cw), in label order, stable inside a group: (order, sizes,
    factors, seeds) of the non-empty groups; group c walks with seed walk_seed (c = 0) or walk_seed + c * _GROUP_MUL."""
    order = np.argsort(cw, kind="stable")
    counts = np.bincount(cw, minlength=len(factors))
    groups = np.flatnonzero(counts)
    return (order, counts[groups], [factors[c] for c in groups],
            [walk_seed if c == 0 else (walk_seed + int(c) * _GROUP_MUL) & _M64 for c in groups])


def _check_resident_clustering(live, clusterer, live_chol, nboot):
    """The arguments that clustering=True with the resident live sets (live=) refuses."""
    if not hasattr(live, "live_runs_step_clustered"):
        raise ValueError("clustering=True with live= needs the resident ensemble's clustered step (GpuRVModel.live_runs_step_clustered)")
    if clusterer is not None:
        raise ValueError("clusterer= does not apply with live=: the resident live sets are clustered on the device")
    if live_chol != "device":
        raise ValueError('live_chol="host" does not work with clustering=True: the resident clustered step whitens on the device')
    from .clustering import MAX_BOOT
    if not 0 <= int(nboot) <= MAX_BOOT:
        raise ValueError(f"nboot must be in [0, {MAX_BOOT}]")


def _check_resident_adaptive(live, distances, live_chol):
    """The arguments that adaptive_nsteps with the resident live sets (live=) refuses."""
    if not hasattr(live, "_live_runs_step_steps"):
        raise ValueError("adaptive_nsteps with live= needs the resident ensemble's step with per-run step counts "
                         "(GpuRVModel.live_runs_step(nsteps=[...], return_distances=True))")
    if distances is not None:
        raise ValueError("distances= does not apply with live=: the resident step measures the walkers on the device")
    if live_chol != "device":
        raise ValueError('live_chol="host" does not work with adaptive_nsteps: the resident step whitens on the device')


def _default_clusterer(clusterer):
    if clusterer is not None:
        return clusterer
    from .clustering import cluster_runs
    return cluster_runs


# ---- the proposal and PolyChord's stop rule (proposal=, precision_criterion=; DESIGN §4i, stepout.py) ---------------------------
def _walk_kwargs(proposal, step_width):
    """The proposal keywords a walker= / walker_runs= / live= call gets: none for the chord walk, so that walker callables
    written before the proposal existed keep working."""
    proposal, step_width = check_proposal(proposal, step_width)
    return {} if proposal == "chord" else {"proposal": proposal, "step_width": step_width}


def _check_precision(precision_criterion):
    if precision_criterion is not None and not (np.isfinite(precision_criterion) and 0.0 < precision_criterion < 1.0):
        raise ValueError("precision_criterion must be in (0, 1)")


def _precision_stop(logz, logx, logl_live, precision_criterion):
    """PolyChord's stop rule: Z_live / (Z_dead + Z_live) < precision_criterion, Z_live = X mean(L_live).  The live log-L are
    summed in ascending order, so that every path (full live array or the resident paths' sorted multiset) gets the same bits."""
    ll = np.sort(np.asarray(logl_live, dtype=np.float64))
    top = ll[-1]
    lz_live = logx + top + np.log(np.mean(np.exp(ll - top)))
    return bool(lz_live - np.logaddexp(logz, lz_live) < np.log(precision_criterion))


def _multiset_step(ll, kdead, new):
    """The live log-L multiset (ascending) of a resident run after an iteration: its kdead lowest died (the values the device
    sort handed down are exactly those), the walkers' new log-L came in."""
    return np.sort(np.concatenate([ll[kdead:], np.asarray(new, dtype=np.float64)]))


def polychord_kwargs(ndim: int, polysettings: Optional[dict] = None) -> dict:
    """The driver keywords (run_nested_slice / run_nested_ensemble) of a run configured with PolyChord's settings
    (settings.polychord_defaults, type-checked as the reference does): nlive; nsteps = num_repeats; clustering =
    do_clustering; precision_criterion; proposal = "stepout".  A nonzero boost_posterior raises ValueError (the drivers return
    the dead points with their weights; they make no boosted posterior).  Ignored: write_resume, read_resume (no resume
    files), feedback (no progress output), and any other key."""
    s = polychord_defaults(ndim, polysettings)
    if s["boost_posterior"] != 0:
        raise ValueError("boost_posterior is not supported: the drivers return the dead points and their weights")
    return {"nlive": s["nlive"], "nsteps": s["num_repeats"], "clustering": s["do_clustering"],
            "precision_criterion": s["precision_criterion"], "proposal": "stepout"}


# ---- step-count adaptation (adaptive_nsteps="move-distance"; DESIGN §4h, adapt.py) -----------------------------------------
def _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, distances):
    """(min_nsteps, max_nsteps, distances) of an adaptive run, or None when adaptation is off."""
    if adaptive_nsteps is None:
        return None
    from . import adapt
    lo, hi = adapt.check_settings(adaptive_nsteps, nsteps, min_nsteps, max_nsteps)
    return lo, hi, (distances if distances is not None else adapt.walk_distances_runs)


def _adapt_counts(entries, distances, wrapped):
    """The counted and far walkers of every entry (one run's iteration each) from ONE `distances` call: an entry is (survivors
    [n, ndim], their cluster labels or None, the factors by label, every walker's label, its start rows, its end rows).  A
    group is a label that has walkers, in label order; its members are the survivors with that label.  Returns (counted [E],
    far [E])."""
    from .adapt import far_counts
    surv, gstart, facs, wg, st, en, wr = [], [0], [], [], [], [], []
    for e, (ua, lab, factors, cw, starts, ends) in enumerate(entries):
        cw = np.asarray(cw, dtype=np.intp)
        groups = np.unique(cw)
        base = len(facs)
        for g in groups:
            rows = ua if lab is None else ua[lab == g]
            surv.append(rows)
            gstart.append(gstart[-1] + len(rows))
            facs.append(factors[g])
        wg.append(base + np.searchsorted(groups, cw))
        st.append(starts); en.append(ends); wr.append(np.full(len(cw), e))
    wg = np.concatenate(wg).astype(np.int32)
    pair, move = distances(np.concatenate(surv), np.array(gstart, dtype=np.int64), np.stack(facs), wrapped,
                           np.concatenate(st), np.concatenate(en), wg)
    return far_counts(pair, move, wg, np.concatenate(wr), len(entries))


# ---- MLFriends region sampling (proposal="region"; DESIGN §4n, region.py) ----------------------------------------------------
_REGION_MUL = 0xA0761D6478BD642F        # region seed of an iteration: seed * _REGION_MUL + it


def _check_region(live, walker, adaptive_nsteps, step_width=1.0):
    """The arguments that proposal="region" refuses."""
    if live is not None:
        raise ValueError('proposal="region" does not work with live=: the resident live sets keep their slice walks '
                         "(region sampling runs in the host-managed drivers only)")
    if walker is not None:
        raise ValueError('proposal="region" finishes short runs through walker_runs= (GpuRVModel.slice_walk_runs) or the host '
                         "walk, not through walker=")
    if adaptive_nsteps is not None:
        raise ValueError('adaptive_nsteps does not apply with proposal="region": a region draw takes no steps')


# ---- the steps every driver is built from -----------------------------------------------------------------------
def _schedule(ndim, nlive, kbatch, nsteps, wrapped):
    """(nlive, kbatch, nsteps, wrapped) of a slice run: the reference's defaults (nlive = 25 ndim, nsteps = 3 ndim) where an
    argument is not given, kbatch = nlive // 4, wrapped as a bool array or None."""
    defaults = ultranest_defaults(ndim)
    nlive = int(nlive or defaults["nlive"])
    kbatch = int(kbatch or max(1, nlive // 4))
    if not 1 <= kbatch < nlive:
        raise ValueError("need 1 <= kbatch < nlive")
    return nlive, kbatch, int(nsteps or defaults["nsteps"]), None if wrapped is None else np.asarray(wrapped, dtype=bool)


def _evaluator(prior, loglike, prior_loglike):
    """cand [n, ndim] -> (theta, logl) as float64 arrays: one prior_loglike call when it is given, else prior, then loglike."""
    def call(cand):
        if prior_loglike is not None:
            ct, cl = prior_loglike(cand)                                # one round trip to the GPU
            return np.asarray(ct, dtype=np.float64), np.asarray(cl, dtype=np.float64)
        ct = np.asarray(prior(cand), dtype=np.float64)
        return ct, np.asarray(loglike(ct), dtype=np.float64)            # one batch = one GPU launch
    return call


def _finish(logz, h, logx, niter, ncall, nlive, kbatch, samples, dead_logl, dead_logw, logl, births, timing=None, nclusters=None,
            nsteps_trace=None, far_fraction=None, region=None):
    """The result of a run that ended with the evidence state (logz, h, logx) and the live log-L `logl`: the live points share
    the remaining prior mass.  dead_logl / dead_logw: lists of arrays in death order.  samples: the finished [dead + live, ndim]
    array (the resident paths fill it from the device), or the list of blocks to stack — the dead blocks, then the live theta.
    births: the list of blocks likewise, or None (a live set without a record).  nclusters / nsteps_trace / far_fraction: the
    per-iteration lists, None when the feature is off.  region: (fallbacks, efficiencies, calls, fallback calls)."""
    logw_live = logx - np.log(max(1, len(logl))) + logl
    logz_final = np.logaddexp(logz, _logaddexp_many(logw_live))
    if isinstance(samples, list):
        samples = np.vstack([a.reshape(-1, samples[-1].shape[1]) for a in samples])
    fallbacks, eff, rcalls, fallback_calls = region or (None, None, None, None)
    return NestedResult(float(logz_final), float(np.sqrt(max(h, 0.0) / nlive)), niter, ncall, float(h), samples,
                        np.concatenate(dead_logl + [logl]), np.concatenate(dead_logw + [logw_live]) - logz_final, timing,
                        None if nclusters is None else np.array(nclusters, dtype=np.int64), nlive=nlive, kbatch=kbatch,
                        logl_birth=None if births is None else np.concatenate(births),
                        nsteps_trace=None if nsteps_trace is None else np.array(nsteps_trace, dtype=np.int64),
                        far_fraction=None if far_fraction is None else np.array(far_fraction, dtype=np.float64),
                        region_fallbacks=fallbacks, region_efficiency=None if eff is None else np.array(eff, dtype=np.float64),
                        region_calls=None if rcalls is None else np.array(rcalls, dtype=np.int64),
                        region_fallback_calls=fallback_calls)


def _stop(logz, logx, top, live_ll, gap, precision_criterion):
    """The stop test: the live points (highest log-L `top`) can add less than dlogz to ln Z — gap = log(expm1(dlogz)) — or,
    when precision_criterion is given, PolyChord's rule on the live log-L multiset live_ll."""
    if precision_criterion is not None:
        return _precision_stop(logz, logx, live_ll, precision_criterion)
    return bool(top + logx < logz + gap)


class _EnsembleRun:
    """The state of one run whose evidence sums the host keeps: its generator, the evidence state, the dead lists, and — for
    the host-managed runs — the live set (u, theta, logl, birth).  The one-run resident paths keep logl alone (host order) or
    not even that (device order), and theta = None."""

    def __init__(self, seed, nlive, ndim, nsteps=None):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.u = self.rng.random((nlive, ndim))
        self.theta = self.logl = None
        self.ncall = nlive
        self.dead_theta, self.dead_logl, self.dead_logw = [], [], []
        self.birth, self.dead_birth = np.full(nlive, -np.inf), []
        self.logz, self.h, self.logx = -np.inf, 0.0, 0.0
        self.it = 0
        self.done = False
        self.timing = {"host_s": 0.0, "walk_s": 0.0, "turns": 0}
        self.order_s = 0.0                          # the seconds of `order` inside die (a one-run path's timing["order_s"])
        self.nclusters = []
        self.nsteps = nsteps                        # this run's step count; adaptive_nsteps: its trace and far fractions
        self.trace, self.fars = [], []
        self.fallbacks, self.fallback_calls, self.eff, self.rcalls = 0, 0, [], []      # proposal="region"

    def stream(self, mul):
        """The seed of this iteration's bootstrap (_BOOT_MUL) or region draw (_REGION_MUL): seed * mul + deaths so far."""
        return (int(self.seed) * mul + self.it) & _M64

    def order(self, kbatch):
        """The host's order step: the stable sort of the live log-L; its first kbatch rows die, and what replaces them is
        born above the highest of them."""
        order = _stable_argsort(self.logl)
        dead = order[:kbatch]
        self.dead_birth.append(self.birth[dead])
        self.birth[dead] = self.logl[dead[-1]]
        return order

    def account(self, dl, kbatch, nlive, dead=None):
        """The evidence sums of an iteration whose dying log-L are dl (ascending), and the dead lists."""
        logw, self.logz, self.h, self.logx = _deaths(self.logz, self.h, self.logx, dl, nlive, kbatch)
        if self.theta is not None:
            self.dead_theta.append(self.theta[dead])                   # (index arrays: already copies)
        self.dead_logl.append(dl); self.dead_logw.append(logw)
        self.it += kbatch

    def die(self, kbatch, nlive):
        """One iteration's deaths of a host-managed run.  Returns (dead rows, lstar, surviving rows in rank order)."""
        t0 = time.perf_counter()
        order = self.order(kbatch)
        self.order_s += time.perf_counter() - t0
        dead = order[:kbatch]
        lstar = self.logl[dead[-1]]
        self.account(self.logl[dead], kbatch, nlive, dead)
        return dead, lstar, order[kbatch:]

    def stopped(self, gap, precision_criterion):
        return _stop(self.logz, self.logx, np.max(self.logl), self.logl, gap, precision_criterion)

    def result(self, nlive, kbatch, clustering, adapting, region=False, one_run=False):
        timing = {"order_s": self.order_s, "step_wait_s": 0.0, "turns": self.timing["turns"]} if one_run else self.timing
        return _finish(self.logz, self.h, self.logx, self.it, self.ncall, nlive, kbatch, self.dead_theta + [self.theta],
                       self.dead_logl, self.dead_logw, self.logl, self.dead_birth + [self.birth], timing,
                       self.nclusters if clustering else None, self.trace if adapting else None, self.fars if adapting else None,
                       (self.fallbacks, self.eff, self.rcalls, self.fallback_calls) if region else None)


@dataclass
class _Turn:
    """One run's part of a lockstep turn: what die returned, then what the proposal draws and groups."""
    run: _EnsembleRun
    dead: np.ndarray                # the rows that died = the rows the new points go to
    lstar: float
    alive: np.ndarray               # the surviving rows in rank order
    start: np.ndarray = None        # the walkers' start rows
    chol: np.ndarray = None         # the whitening factor of all survivors
    walk_seed: int = None
    pick: np.ndarray = None         # start = alive[pick]
    labels: np.ndarray = None       # clustering: the survivors' cluster labels
    factors: list = None            # the whitening factor of every label ([chol] without clusters)
    cw: np.ndarray = None           # every walker's label
    order: np.ndarray = None        # the walkers in group order; sizes, factors and seeds of the non-empty groups (_walk_groups)
    sizes: np.ndarray = None
    gfactors: list = None
    gseeds: list = None
    used: int = 0                   # the likelihood calls of this turn's moves


def _start_runs(seeds, nlive, ndim, nsteps, evaluate):
    """The runs of a lockstep ensemble, their initial live points from ONE evaluate call."""
    runs = [_EnsembleRun(s, nlive, ndim, nsteps) for s in seeds]
    theta, logl = evaluate(np.concatenate([r.u for r in runs]))
    for i, r in enumerate(runs):
        r.theta, r.logl = theta[i * nlive:(i + 1) * nlive].copy(), logl[i * nlive:(i + 1) * nlive].copy()
    return runs


def _lockstep(runs, nlive, kbatch, dlogz, max_iter, max_calls, precision_criterion, propose):
    """The host-managed runs in lockstep until each has met its own stop (dlogz or precision_criterion, max_iter, max_calls):
    per turn the deaths of every running run, ONE propose(turn) that replaces the dead rows of them all and returns the
    seconds of its shared walk or draw calls, then the stop tests.  A run's timing: host_s its own deaths and its share of the
    turn's other host work, walk_s the shared calls it took part in, turns their number."""
    gap = np.log(np.expm1(dlogz))
    while True:
        turn = []
        for r in runs:
            if r.done or not (r.it < max_iter and r.ncall < max_calls):
                r.done = True
                continue
            t0 = time.perf_counter()
            turn.append(_Turn(r, *r.die(kbatch, nlive)))
            r.timing["host_s"] += time.perf_counter() - t0
        if not turn:
            return
        t0 = time.perf_counter()
        walk_s = propose(turn)
        for t in turn:
            t.run.done = t.run.stopped(gap, precision_criterion)
        host_s = (time.perf_counter() - t0 - walk_s) / len(turn)
        for t in turn:
            t.run.timing["host_s"] += host_s
            t.run.timing["walk_s"] += walk_s
            t.run.timing["turns"] += 1


def _host_chord_walk(wu, wt, wl, lstar, chol, wrapped, nsteps, rng, evaluate):
    """nsteps chord moves of every walker inside logL > lstar on the host, drawn from rng; wu / wt / wl are updated in place.
    chol: one whitening factor [ndim, ndim], or one per walker [k, ndim, ndim] (the two products round differently, and each
    is what the device walk of that form computes).  Every shrink round is ONE evaluate call for all unfinished walkers.
    Returns the likelihood calls."""
    k, ndim = wu.shape
    ncall = 0
    for _ in range(nsteps):
        z = rng.standard_normal((k, ndim))
        d = np.einsum("kij,kj->ki", chol, z) if chol.ndim == 3 else z @ chol.T
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        tmin, tmax = _chord(wu, d, wrapped)
        todo = np.arange(k)
        rounds = 0
        while todo.size and rounds < 200:
            t = tmin[todo] + (tmax[todo] - tmin[todo]) * rng.random(todo.size)
            cand = wu[todo] + t[:, None] * d[todo]
            if wrapped is not None:
                cand[:, wrapped] %= 1.0
            cand = np.clip(cand, 0.0, np.nextafter(1.0, 0.0))
            ct, cl = evaluate(cand)
            ncall += todo.size
            ok = cl > lstar
            acc = todo[ok]
            wu[acc], wt[acc], wl[acc] = cand[ok], ct[ok], cl[ok]
            rej = todo[~ok]
            neg = t[~ok] < 0                                        # shrink the bracket towards t = 0
            tmin[rej[neg]] = t[~ok][neg]
            tmax[rej[~neg]] = t[~ok][~neg]
            todo = rej
            rounds += 1
    return ncall


def _one_group(walker):
    """walker= as a walker_runs of one run and one group: group 0 walks with the walk seed itself."""
    def walker_runs(cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds, **pk):
        wu, wt, wl, used = walker(cube, theta, logl, lstar[0], chol[0], wrapped, nsteps, max_rounds, seeds[0], **pk)
        return wu, wt, wl, [int(used)]
    return walker_runs


def _move(turn, wrapped, walker_runs, pk, evaluate):
    """The moves of every entry of the turn, from its start rows into its dead rows (u, theta, logl of its run), each run with
    its own step count: ONE walker_runs call for the (run, cluster) groups of them all, or — without walker_runs — the host
    walk run by run from the run's own generator (the chord walk, or stepout.walk when pk names that proposal).  Adds the
    likelihood calls to the runs and leaves them in the entries' `used`.  Returns the seconds the walk took."""
    t0 = time.perf_counter()
    if walker_runs is None:
        for t in turn:
            r = t.run
            wu, wt, wl = r.u[t.start], r.theta[t.start], r.logl[t.start]
            fac = t.factors[0] if len(t.factors) == 1 else np.stack(t.factors)[t.cw]     # each walker's: its start row's cluster's
            if pk:
                from .stepout import walk as stepout_walk
                t.used = stepout_walk(wu, wt, wl, t.lstar, fac, wrapped, r.nsteps, 200, pk["step_width"], r.rng, evaluate)
            else:
                t.used = _host_chord_walk(wu, wt, wl, t.lstar, fac, wrapped, r.nsteps, r.rng, evaluate)
            r.u[t.dead], r.theta[t.dead], r.logl[t.dead] = wu, wt, wl
            r.ncall += t.used
        return time.perf_counter() - t0
    for t in turn:
        t.order, t.sizes, t.gfactors, t.gseeds = _walk_groups(t.cw, t.factors, t.walk_seed)
    ngroups = [len(t.sizes) for t in turn]
    steps = np.repeat([t.run.nsteps for t in turn], ngroups).astype(np.int32)
    rows = [t.start[t.order] for t in turn]
    cat = np.concatenate if len(turn) > 1 else (lambda parts: parts[0])      # (one run: its rows as they are, no second copy)
    t0 = time.perf_counter()
    wu, wt, wl, used = walker_runs(cat([t.run.u[s] for t, s in zip(turn, rows)]),
                                   cat([t.run.theta[s] for t, s in zip(turn, rows)]),
                                   cat([t.run.logl[s] for t, s in zip(turn, rows)]),
                                   np.concatenate([[0], np.cumsum(np.concatenate([t.sizes for t in turn]))]).astype(np.int64),
                                   np.repeat([t.lstar for t in turn], ngroups), np.stack([f for t in turn for f in t.gfactors]),
                                   wrapped, int(steps[0]) if np.all(steps == steps[0]) else steps, 200,
                                   [s for t in turn for s in t.gseeds], **pk)
    walk_s = time.perf_counter() - t0
    a = g = 0
    for t, n in zip(turn, ngroups):
        r, b = t.run, a + len(t.dead)
        back = t.dead[t.order]                           # the walkers' rows in group order
        r.u[back], r.theta[back], r.logl[back] = wu[a:b], wt[a:b], wl[a:b]
        t.used = int(np.sum(used[g:g + n]))
        r.ncall += t.used
        a, g = b, g + n
    return walk_s


def _cluster_turn(turn, clusterer, wrapped, nboot):
    """clustering=True: the survivors of every run of the turn clustered in ONE clusterer call (which draws nothing from the
    runs' generators); every entry gets the survivors' labels, the factor of every cluster and its walkers' labels."""
    uas = [t.run.u[t.alive] for t in turn]
    run_start = np.concatenate([[0], np.cumsum([len(ua) for ua in uas])]).astype(np.int64)
    labels, ncl, _ = clusterer(np.concatenate(uas), run_start, np.stack([_cluster_scale(ua) for ua in uas]), wrapped, nboot,
                               [t.run.stream(_BOOT_MUL) for t in turn])
    labels = np.asarray(labels, dtype=np.intp)
    for j, t in enumerate(turn):
        t.labels = labels[run_start[j]:run_start[j + 1]]
        t.run.nclusters.append(int(ncl[j]))
        t.factors = _cluster_factors(uas[j], t.labels, int(ncl[j]), t.chol)
        t.cw = t.labels[t.pick]


def _walk_proposal(kbatch, wrapped, walker_runs, clusterer, nboot, adapting, pk, evaluate):
    """The slice walk as _lockstep's proposal.  Per run: the whitening from the survivors, then from the run's generator the
    start rows and — for walker_runs only; the host walk draws its moves from the generator itself — the walk seed.  Then the
    clustering (clusterer given), the moves (_move), and the step-count rule from ONE distances call (adapting)."""
    def propose(turn):
        for t in turn:
            r = t.run
            t.chol = _whitening(r.u[t.alive])
            t.pick = r.rng.integers(0, len(t.alive), kbatch)
            t.start = t.alive[t.pick]
            if walker_runs is not None:
                t.walk_seed = int(r.rng.integers(0, 2 ** 62))
            t.factors, t.cw = [t.chol], np.zeros(kbatch, dtype=np.intp)
        if clusterer is not None:
            _cluster_turn(turn, clusterer, wrapped, nboot)
        if adapting:
            starts = [t.run.u[t.start] for t in turn]
        walk_s = _move(turn, wrapped, walker_runs, pk, evaluate)
        if adapting:
            from .adapt import far_fraction, next_nsteps
            c, f = _adapt_counts([(t.run.u[t.alive], t.labels, t.factors, t.cw, s, t.run.u[t.dead]) for t, s in zip(turn, starts)],
                                 adapting[2], wrapped)
            for j, t in enumerate(turn):
                r = t.run
                r.trace.append(r.nsteps)
                r.fars.append(float(far_fraction(f[j], c[j])))
                r.nsteps = next_nsteps(r.nsteps, int(f[j]), int(c[j]), adapting[0], adapting[1])
        return walk_s
    return propose


def _region_proposal(kbatch, wrapped, walker_runs, clusterer, nboot, region_runs, cap, evaluate):
    """MLFriends region sampling as _lockstep's proposal: ONE clusterer call (every running run's scale and radius2) and ONE
    region_runs call (kbatch draws of every running run), then the chord walk (_move) for whatever a run is short of — only
    such a run draws from its generator: the start rows, then the walk seed."""
    def propose(turn):
        uas = [t.run.u[t.alive] for t in turn]
        run_start = np.concatenate([[0], np.cumsum([len(ua) for ua in uas])]).astype(np.int64)
        surv = np.concatenate(uas)
        scales = np.stack([_cluster_scale(ua) for ua in uas])
        _lab, ncl, radius2 = clusterer(surv, run_start, scales, wrapped, nboot, [t.run.stream(_BOOT_MUL) for t in turn])
        t1 = time.perf_counter()
        cu, ct, cl, nfound, ncalls = region_runs(surv, run_start, scales, np.asarray(radius2, dtype=np.float64),
                                                 np.array([t.lstar for t in turn], dtype=np.float64),
                                                 [t.run.stream(_REGION_MUL) for t in turn], kbatch,
                                                 wrapped=wrapped, max_candidates=cap)
        short = []
        for j, t in enumerate(turn):
            r, nf, nc = t.run, int(nfound[j]), int(ncalls[j])
            r.nclusters.append(int(ncl[j]))
            r.rcalls.append(nc)
            r.eff.append(nf / nc if nc > 0 else float("nan"))
            r.ncall += nc
            rows = t.dead[:nf]
            r.u[rows], r.theta[rows], r.logl[rows] = cu[j, :nf], ct[j, :nf], cl[j, :nf]
            if nf < kbatch:
                k = kbatch - nf
                start = t.alive[r.rng.integers(0, len(t.alive), k)]
                chol = _whitening(uas[j])
                short.append(_Turn(r, t.dead[nf:], t.lstar, t.alive, start, chol, int(r.rng.integers(0, 2 ** 62)),
                                   factors=[chol], cw=np.zeros(k, dtype=np.intp)))
                r.fallbacks += k
        if short:
            _move(short, wrapped, walker_runs, {}, evaluate)
            for t in short:
                t.run.fallback_calls += t.used
        return time.perf_counter() - t1
    return propose


def _walk_ensemble(prior, loglike, prior_loglike, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                   walker_runs, clustering, nboot, clusterer, adaptive_nsteps, min_nsteps, max_nsteps, distances, pk,
                   precision_criterion, one_run=False):
    """The host-managed slice walk of run_nested_slice (one seed, one_run: its timing keys) and run_nested_ensemble.  The
    initial live points are one prior, then one loglike call, even when prior_loglike is given (the host walk's rounds use it)."""
    clusterer = _default_clusterer(clusterer) if clustering else None
    nlive, kbatch, nsteps, wrapped = _schedule(ndim, nlive, kbatch, nsteps, wrapped)
    adapting = _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, distances)
    runs = _start_runs(seeds, nlive, ndim, nsteps, _evaluator(prior, loglike, None))
    _lockstep(runs, nlive, kbatch, dlogz, max_iter, max_calls, precision_criterion,
              _walk_proposal(kbatch, wrapped, walker_runs, clusterer, nboot, adapting, pk, _evaluator(prior, loglike, prior_loglike)))
    return [r.result(nlive, kbatch, clustering, bool(adapting), one_run=one_run) for r in runs]


def _region_ensemble(prior, loglike, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, walker_runs, nboot,
                     clusterer, region_runs, region_max_candidates, precision_criterion, prior_loglike=None):
    """proposal="region" of run_nested_slice (one seed) and run_nested_ensemble.  Every draw of a run depends on its own seed,
    iteration and survivors alone, so result[r] is the one-seed run bit for bit.  The initial live points are one call of the
    evaluator the draws use (prior_loglike when it is given)."""
    from . import region as _region
    clusterer = _default_clusterer(clusterer)
    nlive, kbatch, nsteps, wrapped = _schedule(ndim, nlive, kbatch, nsteps, wrapped)
    cap = int(_region.DEFAULT_MAX_CANDIDATES if region_max_candidates is None else region_max_candidates)
    if cap < 0:
        raise ValueError("region_max_candidates must not be negative")
    evaluate = _evaluator(prior, loglike, prior_loglike)
    if region_runs is None:
        def region_runs(surv, run_start, scale, radius2, lstar, rseeds, kdraw, wrapped=None, max_candidates=cap):
            return _region.draw_runs(surv, run_start, scale, radius2, lstar, rseeds, kdraw, evaluate, wrapped=wrapped,
                                     max_candidates=max_candidates)
    runs = _start_runs(seeds, nlive, ndim, nsteps, evaluate)
    _lockstep(runs, nlive, kbatch, dlogz, max_iter, max_calls, precision_criterion,
              _region_proposal(kbatch, wrapped, walker_runs, clusterer, nboot, region_runs, cap, evaluate))
    return [r.result(nlive, kbatch, True, False, region=True) for r in runs]


def _slice_resident(live, ndim, seed, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, live_chol, pk,
                    precision_criterion):
    """run_nested_slice(live=model), one run: the live set resident on the device (GpuRVModel.live_init / live_step).  Three
    forms.  live_chol="host" mirrors the cube rows, whitens on the host and waits for the step.  live_chol="device" keeps the
    log-L and the order on the host; the walk needs nothing of the iteration's evidence sums, so it starts first — on a helper
    thread (the C call releases the interpreter lock) — and the sums run on the host while the GPU walks.  With
    GpuRVModel.live_sort the ORDER is on the device as well: no per-point state on the host at all — per iteration the log-L
    of the dying points comes down (the evidence sums need them) and ranks go up (the draw the host order's alive[...] makes)."""
    nlive, kbatch, nsteps, wrapped = _schedule(ndim, nlive, kbatch, nsteps, wrapped)
    if live_chol not in ("device", "host"):
        raise ValueError(live_chol)
    run = _EnsembleRun(seed, nlive, ndim)
    rng, mirror = run.rng, live_chol == "host"
    run.logl = live.live_init(run.u)
    if not mirror:
        run.u = None                                   # no host mirror of the rows at all
    device_order = not mirror and hasattr(live, "live_sort")
    top = float(np.max(run.logl)) if device_order else None
    # precision_criterion on the device-ordered path: the live log-L multiset, from the values that come down anyway
    live_ll = np.sort(run.logl) if device_order and precision_criterion is not None else None
    timing = {"order_s": 0.0, "step_wait_s": 0.0, "turns": 0}
    gap = np.log(np.expm1(dlogz))
    while run.it < max_iter and run.ncall < max_calls:
        timing["turns"] += 1
        t0 = time.perf_counter()
        if device_order:
            order = dead = None
            dl, lstar, top = live.live_sort(kbatch)
        else:
            order = run.order(kbatch)
            dead = order[:kbatch]
            dl, lstar = run.logl[dead], run.logl[dead[-1]]
        timing["order_s"] += time.perf_counter() - t0
        if mirror:
            chol = _whitening(run.u[order[kbatch:]])
        start = rng.integers(0, nlive - kbatch, kbatch)
        if not device_order:
            start = order[kbatch:][start]
        step = (order, kbatch, start, lstar, wrapped, nsteps, 200, int(rng.integers(0, 2 ** 62)))
        pending = None if mirror else _helper().submit(live.live_step, *step, **pk)
        run.account(dl, kbatch, nlive)
        if mirror:
            # order and start rows up, the new log-L of the replaced rows down, and the mirror of the rows
            wl, used = live.live_step(*step, chol=chol, **pk)
        else:
            t0 = time.perf_counter()
            wl, used = pending.result()
            timing["step_wait_s"] += time.perf_counter() - t0
        run.ncall += int(used)
        if device_order:
            top = max(top, float(np.max(wl)))                     # the survivors' highest and the newcomers'
            if live_ll is not None:
                live_ll = _multiset_step(live_ll, kbatch, wl)
            if _stop(run.logz, run.logx, top, live_ll, gap, precision_criterion):
                break
            continue
        run.logl[dead] = wl
        if mirror:
            run.u = live.live_get()[0]
        if run.stopped(gap, precision_criterion):
            break
    if device_order:
        run.logl = live.live_get(cube=False, theta=False)[2]              # the live points' log-L: once, at the end
    if hasattr(live, "live_dead_count"):
        # the samples come down once, straight into the array that is returned: dead points first, then the live set
        ndead = live.live_dead_count()
        samples = np.empty((ndead + nlive, ndim))
        live.live_dead(theta_out=samples[:ndead])
        live.live_get(cube=False, logl=False, theta_out=samples[ndead:])
    else:
        samples = [live.live_dead()[0], live.live_get()[1]]
    if hasattr(live, "live_births"):
        births = live.live_births()                           # the device's own record (it chose the dying rows)
    else:                                                     # (device order without it: the host never saw which rows died)
        births = None if device_order else run.dead_birth + [run.birth]
    return _finish(run.logz, run.h, run.logx, run.it, run.ncall, nlive, kbatch, samples, run.dead_logl, run.dead_logw, run.logl,
                   births, timing)


def run_nested_slice(prior: Callable, loglike: Callable, ndim: int, nlive: Optional[int] = None, kbatch: Optional[int] = None,
                     nsteps: Optional[int] = None, dlogz: float = 0.5, max_iter: int = 10_000_000,
                     max_calls: int = 50_000_000, wrapped=None, seed: int = 0,
                     prior_loglike: Optional[Callable] = None, walker: Optional[Callable] = None,
                     live=None, live_chol: str = "device", clustering: bool = False, nboot: int = 30,
                     clusterer: Optional[Callable] = None, walker_runs: Optional[Callable] = None,
                     adaptive_nsteps: Optional[str] = None, min_nsteps: Optional[int] = None, max_nsteps: Optional[int] = None,
                     distances: Optional[Callable] = None, proposal: str = "chord", step_width: float = 1.0,
                     precision_criterion: Optional[float] = None, region_runs: Optional[Callable] = None,
                     region_max_candidates: Optional[int] = None) -> NestedResult:
    """Nested sampling with `kbatch` deaths per iteration and batched hit-and-run slice sampling.

    `prior_loglike(cubes) -> (theta, logl)`, if given, replaces the prior + loglike pair inside the loop
    (GpuRVModel.prior_loglike_batch: one upload, two launches, one download per round).
    `walker(cube, theta, logl, lstar, chol, wrapped, nsteps, max_rounds, seed) -> (cube, theta, logl, ncalls)`,
    if given, runs all `nsteps` moves of all replacement walkers in ONE call (GpuRVModel.slice_walk: the whole
    walk — directions, chords, candidates, prior transform, log-L, accept / shrink — stays on the GPU).
    `live`, if given (a GpuRVModel), keeps the LIVE SET ITSELF on the GPU (GpuRVModel.live_init / live_step: rvll_live_*):
    unit-cube rows, theta and log-L of the live points and of the points that died never leave HBM during the run; per
    iteration the host sends the sort order and the walkers' start rows and reads back the new log-L — what it needs
    for the sort and the evidence sum.  `prior` / `loglike` / `walker` are then unused.  live_chol="device" (default) takes
    the whitening from the surviving rows' covariance summed on the device; "host" mirrors the cube rows on the host
    and factors them exactly as the other paths do — slower, and bit-identical to `walker=model.slice_walk` for a seed
    (the equivalence test's mode).

    Each iteration removes the `kbatch` lowest live points in order (the live count shrinks nlive,
    nlive-1, ... while they die, as in dynamic nested sampling), then draws `kbatch` replacements above
    the highest removed likelihood: walkers start from random surviving live points and take `nsteps`
    slice moves along random directions whitened by the live-point covariance; a slice starts as the whole
    chord inside the unit cube (circular `wrapped` parameters wrap instead) and is shrunk towards the
    current position until a proposal is accepted.  Every shrink round evaluates ALL unfinished walkers in
    one vectorized callback call — one prior + log-L launch on the GPU.  Defaults follow the reference's
    UltraNest wrapper (evidence_amd/settings.py: nlive = 25 ndim, nsteps = 3 ndim, dlogz = 0.5;
    evidence/ultranest/__init__.py:333-338) and :159-163 (wrapped parameters).

    `clustering=True` (the reference's PolyChord do_clustering / UltraNest's MLFriends regions) clusters the survivors of
    every iteration (MLFriends with `nboot` bootstraps; `clusterer` = clustering.cluster_runs by default, or
    GpuRVModel.cluster_runs) and whitens every walker's directions with the covariance of the cluster its start row is in.
    The draws of the run's generator are those of clustering=False, so a run that finds one cluster every iteration is the
    unclustered run bit for bit.  `walker_runs` (GpuRVModel.slice_walk_runs) then walks the walkers grouped by cluster in
    one call; `walker` has a single factor and cannot be combined with clustering.

    With `live` as well, the clustering runs on the device (GpuRVModel.live_runs_step_clustered): the run is the
    one-run resident ENSEMBLE, run_nested_ensemble(None, None, ndim, [seed], live=live, clustering=True, ...)[0], with the
    ensemble's draws, results and `timing` keys; the model is left holding that ensemble (live_runs_*), not a one-run live set.
    `clusterer` (the device clusters) and live_chol="host" (the device whitens) are refused then.

    adaptive_nsteps="move-distance" (UltraNest's adaptive_nsteps='move-distance'; DESIGN §4h, adapt.py) changes every run's
    step count from one iteration to the next by how far its walkers got from their start rows, measured against the mean
    distance between the survivors of their group, within [min_nsteps (default: nsteps), max_nsteps (default 1000)].
    `distances` (adapt.walk_distances_runs by default, or GpuRVModel.walk_distances_runs) gives those distances, one call per
    iteration.  With `live` the run is the one-run resident ensemble, whose step measures the walkers on the device
    (`distances` is refused).  The rule draws nothing, so every draw is that of the same run without adaptation;
    the results gain `nsteps_trace` and `far_fraction`.

    proposal="stepout" (stepout.py) walks with PolyChord's stepping-out slice proposal instead of the chord walk:
    directions along a random orthonormal basis cycled every ndim moves, brackets `step_width` whitened units wide that step
    out while their ends are inside the slice.  The host walk runs stepout.walk; walker= / walker_runs= / live= get
    proposal= and step_width= (only when the proposal is not "chord").  precision_criterion (PolyChord's stop rule) replaces
    the dlogz test: stop when Z_live / (Z_dead + Z_live) < precision_criterion, Z_live = X mean(L_live).
    polychord_kwargs(ndim, polysettings) gives the keywords of a run configured with PolyChord's settings.

    proposal="region" (region.py) draws the replacements by MLFriends region sampling instead of a walk: uniform
    rejection sampling from the union of the balls around the survivors, every accepted point an exact, independent draw from
    the prior inside the contour.  Per iteration `clusterer` (clustering.cluster_runs, or GpuRVModel.cluster_runs) gives the
    survivors' MLFriends radius (`nboot` bootstraps) and `region_runs` (region.draw_runs on the callbacks by default, or
    GpuRVModel.region_draw_runs) draws the kbatch points from at most `region_max_candidates` candidates (default
    region.DEFAULT_MAX_CANDIDATES).  Points a draw stays short of come from the chord walk (`walker_runs`, or the host walk)
    and are counted in the result's `region_fallbacks`; `region_efficiency` and `region_calls` hold every iteration's
    accepted / calls and calls.  The run is run_nested_ensemble(..., [seed], proposal="region")[0].  Not with live= (the
    resident live sets keep their walks), walker= or adaptive_nsteps."""
    if proposal == "region":
        _check_region(live, walker, adaptive_nsteps)
        _check_precision(precision_criterion)
        return _region_ensemble(prior, loglike, ndim, [int(seed)], nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                walker_runs, nboot, clusterer, region_runs, region_max_candidates, precision_criterion,
                                prior_loglike=prior_loglike)[0]
    pk = _walk_kwargs(proposal, step_width)
    _check_precision(precision_criterion)
    if clustering and walker is not None:
        raise ValueError("walker= has one whitening factor for all walkers: with clustering=True pass walker_runs= "
                         "(GpuRVModel.slice_walk_runs)")
    if live is not None and (clustering or adaptive_nsteps is not None):       # the one-run resident ensemble
        if adaptive_nsteps is not None:
            _check_resident_adaptive(live, distances, live_chol)
        if clustering:
            _check_resident_clustering(live, clusterer, live_chol, nboot)
        return _ensemble_resident(live, ndim, [int(seed)], nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                  clustering=clustering, nboot=nboot, adaptive_nsteps=adaptive_nsteps, min_nsteps=min_nsteps,
                                  max_nsteps=max_nsteps, pk=pk, precision_criterion=precision_criterion)[0]
    if walker is not None and walker_runs is not None:
        raise ValueError("pass walker= or walker_runs=, not both")
    if live is not None:
        return _slice_resident(live, ndim, seed, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, live_chol, pk,
                               precision_criterion)
    return _walk_ensemble(prior, loglike, prior_loglike, ndim, [seed], nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                          walker_runs if walker is None else _one_group(walker), clustering, nboot, clusterer, adaptive_nsteps,
                          min_nsteps, max_nsteps, distances, pk, precision_criterion, one_run=True)[0]


def run_nested_ensemble(prior: Callable, loglike: Callable, ndim: int, seeds, nlive: Optional[int] = None,
                        kbatch: Optional[int] = None, nsteps: Optional[int] = None, dlogz: float = 0.5,
                        max_iter: int = 10_000_000, max_calls: int = 50_000_000, wrapped=None,
                        walker_runs: Optional[Callable] = None, clustering: bool = False, nboot: int = 30,
                        clusterer: Optional[Callable] = None, live=None, adaptive_nsteps: Optional[str] = None,
                        min_nsteps: Optional[int] = None, max_nsteps: Optional[int] = None,
                        distances: Optional[Callable] = None, proposal: str = "chord", step_width: float = 1.0,
                        precision_criterion: Optional[float] = None, region_runs: Optional[Callable] = None,
                        region_max_candidates: Optional[int] = None) -> list:
    """len(seeds) independent runs of run_nested_slice in lockstep, their walks in ONE call per iteration.

    The reference's FIP workflow repeats independent runs of every model and takes the median and spread of ln Z over them
    (evidence/fip_criterion.py).  One run's walk is a few hundred walkers, far too few to fill a GPU, and a chain of
    dependent moves whose time is set by latency: the walkers of R runs walk side by side for about the cost of one.
    `walker_runs(cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds) -> (cube, theta, logl,
    ncalls[R])` walks the rows run_start[r] .. run_start[r + 1] of run r inside logL > lstar[r] with chol[r] and seeds[r]
    (GpuRVModel.slice_walk_runs).

    The initial live points of all runs are one prior + loglike call.  Every iteration then does, run by run, the
    bookkeeping of run_nested_slice's `walker=` path — sort, deaths, evidence and information sums, whitening from the
    survivors, start rows and walk seed drawn from the run's own default_rng(seed) — and makes one `walker_runs` call for
    the walkers of every run that is still going.  A run that meets its own stop (dlogz, max_iter, max_calls) leaves the
    lockstep.  result[r] is run_nested_slice(prior, loglike, ndim, seed=seeds[r], walker=<the same walk for one run>,
    same settings) bit for bit; its `timing` holds the host seconds of its own bookkeeping, the seconds of the shared walk
    calls it took part in, and their number.

    clustering=True clusters the survivors of every running run in ONE `clusterer` call per iteration and walks the
    (run, cluster) groups of walkers in one `walker_runs` call; result[r] is then run_nested_slice(..., clustering=True,
    walker_runs=...) for seed r, bit for bit, and the runs' timing counts the clustering as host time.

    `live` (a GpuRVModel) keeps the live sets of ALL runs resident on the device (GpuRVModel.live_runs_*: rvll_live_runs_*,
    DESIGN §4d): per iteration one call sorts every running run and one call whitens and walks them all; `prior`, `loglike`
    and `walker_runs` are unused and may be None.  result[r] is then run_nested_slice(None, None, ndim, seed=seeds[r],
    live=<a model of that run alone>, same settings) bit for bit, and its timing holds its share of the host seconds of each
    turn (sort, draws, evidence sums), the seconds of the shared step calls it took part in, and their number.  Not with
    walker_runs.  With clustering=True every step clusters the survivors of every running run on the device
    (GpuRVModel.live_runs_step_clustered): the runs' draws are those of the unclustered ensemble, the bootstrap seed
    of a run's iteration is the host clustered path's, and result[r] is run_nested_slice(None, None, ndim, seed=seeds[r],
    live=..., clustering=True), with `nclusters`; `clusterer` is refused (the device clusters).

    adaptive_nsteps="move-distance" (with min_nsteps, max_nsteps, distances as run_nested_slice takes them): every run keeps
    its own step count, the walk call gets them per group (an int when they are all equal), and one `distances` call per
    iteration measures the walkers of every run; result[r] is run_nested_slice(..., adaptive_nsteps=...) for seed r, bit for
    bit.  With live= the resident step takes the per-run counts and returns the distances from the device rows
    (GpuRVModel.live_runs_step(nsteps=[...], return_distances=True)); result[r] is then the standalone resident adaptive run.

    proposal= / step_width= / precision_criterion= as run_nested_slice takes them: result[r] is the standalone run of seed r with
    the same keywords, bit for bit.

    proposal="region" (with region_runs=, region_max_candidates=, nboot, clusterer as run_nested_slice takes them): one clusterer
    call and one region_runs call per iteration for all running runs; walker_runs is optional then (it finishes short runs;
    without it the host walk does).  result[r] is run_nested_slice(..., seed=seeds[r], proposal="region") bit for bit.  Not
    with live=."""
    if proposal == "region":
        _check_region(live, None, adaptive_nsteps)
    else:
        pk = _walk_kwargs(proposal, step_width)
    _check_precision(precision_criterion)
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("need at least one seed")
    if proposal == "region":
        return _region_ensemble(prior, loglike, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                walker_runs, nboot, clusterer, region_runs, region_max_candidates, precision_criterion)
    if adaptive_nsteps is not None and live is not None:
        _check_resident_adaptive(live, distances, "device")
    if live is not None:
        if clustering:
            _check_resident_clustering(live, clusterer, "device", nboot)
        if walker_runs is not None:
            raise ValueError("pass walker_runs= or live=, not both")
        return _ensemble_resident(live, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                  clustering=clustering, nboot=nboot, adaptive_nsteps=adaptive_nsteps, min_nsteps=min_nsteps,
                                  max_nsteps=max_nsteps, pk=pk, precision_criterion=precision_criterion)
    if walker_runs is None:
        raise ValueError("walker_runs is required (GpuRVModel.slice_walk_runs)")
    return _walk_ensemble(prior, loglike, None, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, walker_runs,
                          clustering, nboot, clusterer, adaptive_nsteps, min_nsteps, max_nsteps, distances, pk, precision_criterion)


def _ensemble_resident(live, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, clustering=False, nboot=30,
                       adaptive_nsteps=None, min_nsteps=None, max_nsteps=None, pk=None, precision_criterion=None):
    """run_nested_ensemble(live=model): the device-order form of _slice_resident for every seed, the runs' live sets resident
    side by side (run r = rows r nlive .. r nlive + nlive - 1 of the ensemble), their bookkeeping vectorised across runs.
    clustering: the clustered step, with run r's bootstrap seed (seeds[r] _BOOT_MUL + deaths after this iteration) mod 2^64 —
    what run_nested_slice's host clustered path passes.  adaptive_nsteps: every run walks with its own step count, and the step
    returns the walkers' distances from the device rows (GpuRVModel.live_runs_step(nsteps=[...], return_distances=True))."""
    nlive, kbatch, nsteps, wrapped = _schedule(ndim, nlive, kbatch, nsteps, wrapped)
    adapting = _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, None)
    R = len(seeds)
    steps = np.full(R, nsteps, dtype=np.int64)
    trace, fars = [[] for _ in range(R)], [[] for _ in range(R)]
    rngs = [np.random.default_rng(s) for s in seeds]
    pk = pk or {}
    ll0 = live.live_runs_init(np.concatenate([g.random((nlive, ndim)) for g in rngs]), R)
    # precision_criterion: every run's live log-L multiset, kept from the values that come down anyway (init, the sort's dying
    # values, the step's new log-L)
    live_ll = [np.sort(ll0[r]) for r in range(R)] if precision_criterion is not None else None
    ncall = np.full(R, nlive, dtype=np.int64)
    logz, h = np.full(R, -np.inf), np.zeros(R)
    logx_run, niter = np.zeros(R), np.zeros(R, dtype=np.int64)
    done = np.zeros(R, dtype=bool)
    timing = [{"host_s": 0.0, "walk_s": 0.0, "turns": 0} for _ in range(R)]
    ncls = [[] for _ in range(R)]
    stop_gap = np.log(np.expm1(dlogz))
    it, logx = 0, 0.0                               # every running run is at the same iteration
    turns = []                                      # (runs, dying log-L [A, kbatch], their log-weights) of every turn
    while it < max_iter:
        act = np.flatnonzero(~done & (ncall < max_calls))
        if not act.size:
            break
        t0 = time.perf_counter()
        dl, lstar, top = live.live_runs_sort(act, kbatch)
        ranks = np.empty((act.size, kbatch), dtype=np.int64)
        walk_seeds = []
        for j, r in enumerate(act):                 # the draws of the standalone run, from the run's own generator
            ranks[j] = rngs[r].integers(0, nlive - kbatch, kbatch)
            walk_seeds.append(int(rngs[r].integers(0, 2 ** 62)))
        t1 = time.perf_counter()
        st = steps[act] if adapting else nsteps
        dist = {"return_distances": True} if adapting else {}
        if clustering:
            boot = [(seeds[r] * _BOOT_MUL + it + kbatch) & _M64 for r in act]
            wl, used, ncl, *md = live.live_runs_step_clustered(act, kbatch, ranks, lstar, wrapped, st, 200, walk_seeds, nboot, boot,
                                                               **dist, **pk)
            for j, r in enumerate(act):
                ncls[r].append(int(ncl[j]))
        else:
            wl, used, *md = live.live_runs_step(act, kbatch, ranks, lstar, wrapped, st, 200, walk_seeds, **dist, **pk)
        t2 = time.perf_counter()
        if adapting:
            from .adapt import far_fraction, next_nsteps
            move, pair = md
            counted = ~np.isnan(pair)
            c = np.count_nonzero(counted, axis=1)
            f = np.count_nonzero(counted & (move > pair), axis=1)
            ff = far_fraction(f, c)
            for j, r in enumerate(act):
                trace[r].append(int(steps[r]))
                fars[r].append(float(ff[j]))
            steps[act] = next_nsteps(steps[act], f, c, adapting[0], adapting[1])
        logw, logz[act], h[act], logx = _deaths_runs(logz[act], h[act], logx, dl, nlive, kbatch)
        turns.append((act, dl, logw))
        it += kbatch
        ncall[act] += used
        wmax = np.max(wl, axis=1)
        top = np.where(wmax > top, wmax, top)       # max(top, max(wl)) as the standalone run takes it
        if precision_criterion is not None:
            for j, r in enumerate(act):
                live_ll[r] = _multiset_step(live_ll[r], kbatch, wl[j])
                if _precision_stop(logz[r], logx, live_ll[r], precision_criterion):
                    done[r] = True
        else:
            done[act[top + logx < logz[act] + stop_gap]] = True
        niter[act], logx_run[act] = it, logx
        host = (time.perf_counter() - t2 + t1 - t0) / act.size
        for r in act:
            tr = timing[r]
            tr["host_s"] += host
            tr["walk_s"] += t2 - t1
            tr["turns"] += 1
    dead_logl, dead_logw = [[] for _ in range(R)], [[] for _ in range(R)]
    for act, dl, logw in turns:
        for j, r in enumerate(act):
            dead_logl[r].append(dl[j]); dead_logw[r].append(logw[j])
    out = []
    for r in range(R):
        logl = live.live_runs_get(r, cube=False, theta=False)[2]
        ndead = live.live_runs_dead_count(r)
        all_theta = np.empty((ndead + nlive, ndim))
        live.live_runs_dead(r, theta_out=all_theta[:ndead])
        live.live_runs_get(r, cube=False, logl=False, theta_out=all_theta[ndead:])
        out.append(_finish(logz[r], h[r], logx_run[r], int(niter[r]), int(ncall[r]), nlive, kbatch, all_theta, dead_logl[r],
                           dead_logw[r], logl, live.live_runs_births(r) if hasattr(live, "live_runs_births") else None, timing[r],
                           ncls[r] if clustering else None, trace[r] if adapting else None, fars[r] if adapting else None))
    return out
