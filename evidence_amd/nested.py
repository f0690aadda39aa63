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
    # final live points share the remaining prior mass
    logw_live = logx - np.log(max(1, len(logl))) + logl
    logz_final = np.logaddexp(logz, _logaddexp_many(logw_live))
    all_theta = np.vstack([np.array(dead_theta).reshape(-1, ndim), theta])
    all_logl = np.concatenate([dead_logl, logl])
    all_logw = np.concatenate([dead_logw, logw_live]) - logz_final
    return NestedResult(float(logz_final), float(np.sqrt(max(h, 0.0) / nlive)), it, ncall, float(h),
                        all_theta, all_logl, all_logw, nlive=nlive, kbatch=1,
                        logl_birth=np.concatenate([np.array(dead_birth, dtype=np.float64), birth]))


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
def _stop(logz, logx, logl, dlogz, precision_criterion):
    """The stop test of a path that holds the whole live log-L array: the dlogz test, or PolyChord's rule when given."""
    if precision_criterion is not None:
        return _precision_stop(logz, logx, logl, precision_criterion)
    return bool(np.max(logl) + logx < logz + np.log(np.expm1(dlogz)))


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


def _host_chord_walk(wu, wt, wl, lstar, chol, wrapped, nsteps, rng, evaluate):
    """nsteps chord moves of every walker inside logL > lstar, as run_nested_slice's host loop makes them (one whitening
    factor); wu / wt / wl are updated in place.  Returns the likelihood calls."""
    k, ndim = wu.shape
    ncall = 0
    for _ in range(nsteps):
        z = rng.standard_normal((k, ndim))
        d = z @ chol.T
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
            neg = t[~ok] < 0
            tmin[rej[neg]] = t[~ok][neg]
            tmax[rej[~neg]] = t[~ok][~neg]
            todo = rej
            rounds += 1
    return ncall


def _region_ensemble(prior, loglike, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, walker_runs, nboot,
                     clusterer, region_runs, region_max_candidates, precision_criterion, prior_loglike=None):
    """proposal="region" of run_nested_slice (one seed) and run_nested_ensemble: the runs in lockstep, per iteration ONE
    clusterer call (every running run's scale and MLFriends radius2) and ONE region_runs call (kbatch draws of every running
    run), then the chord walk for whatever a run is short of.  Every draw of a run depends on its own seed, iteration and
    survivors alone, so result[r] is the one-seed run bit for bit."""
    from . import region as _region
    clusterer = _default_clusterer(clusterer)
    defaults = ultranest_defaults(ndim)
    nlive = int(nlive or defaults["nlive"])
    kbatch = int(kbatch or max(1, nlive // 4))
    if not 1 <= kbatch < nlive:
        raise ValueError("need 1 <= kbatch < nlive")
    nsteps = int(nsteps or defaults["nsteps"])
    cap = int(_region.DEFAULT_MAX_CANDIDATES if region_max_candidates is None else region_max_candidates)
    if cap < 0:
        raise ValueError("region_max_candidates must not be negative")
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool)

    def evaluate(cand):
        if prior_loglike is not None:
            ct, cl = prior_loglike(cand)
            return np.asarray(ct, dtype=np.float64), np.asarray(cl, dtype=np.float64)
        ct = np.asarray(prior(cand), dtype=np.float64)
        return ct, np.asarray(loglike(ct), dtype=np.float64)

    if region_runs is None:
        def region_runs(surv, run_start, scale, radius2, lstar, rseeds, kdraw, wrapped=None, max_candidates=cap):
            return _region.draw_runs(surv, run_start, scale, radius2, lstar, rseeds, kdraw, evaluate, wrapped=wrapped,
                                     max_candidates=max_candidates)
    runs = [_EnsembleRun(s, nlive, ndim) for s in seeds]
    for r in runs:
        r.fallbacks, r.fallback_calls, r.eff, r.rcalls = 0, 0, [], []
    theta, logl = evaluate(np.concatenate([r.u for r in runs]))
    for i, r in enumerate(runs):
        r.theta, r.logl = theta[i * nlive:(i + 1) * nlive].copy(), logl[i * nlive:(i + 1) * nlive].copy()
    stop_gap = np.log(np.expm1(dlogz))
    while True:
        turn = []                                   # (run, dead rows, lstar, surviving rows in rank order)
        for r in runs:
            if r.done:
                continue
            if not (r.it < max_iter and r.ncall < max_calls):
                r.done = True
                continue
            t0 = time.perf_counter()
            order = _stable_argsort(r.logl)
            dead = order[:kbatch]
            lstar = r.logl[dead[-1]]
            dl = r.logl[dead]
            logw, r.logz, r.h, r.logx = _deaths(r.logz, r.h, r.logx, dl, nlive, kbatch)
            r.dead_theta.append(r.theta[dead])
            r.dead_logl.append(dl); r.dead_logw.append(logw)
            r.dead_birth.append(r.birth[dead])
            r.birth[dead] = lstar
            r.it += kbatch
            turn.append((r, dead, lstar, order[kbatch:]))
            r.timing["host_s"] += time.perf_counter() - t0
        if not turn:
            break
        t0 = time.perf_counter()
        uas = [r.u[alive] for r, _d, _l, alive in turn]
        run_start = np.concatenate([[0], np.cumsum([len(ua) for ua in uas])]).astype(np.int64)
        surv = np.concatenate(uas)
        scales = np.stack([_cluster_scale(ua) for ua in uas])
        _lab, ncl, radius2 = clusterer(surv, run_start, scales, wrapped, nboot, [(r.seed * _BOOT_MUL + r.it) & _M64 for r, *_x in turn])
        t1 = time.perf_counter()
        cu, ct, cl, nfound, ncalls = region_runs(surv, run_start, scales, np.asarray(radius2, dtype=np.float64),
                                                 np.array([t[2] for t in turn], dtype=np.float64),
                                                 [(r.seed * _REGION_MUL + r.it) & _M64 for r, *_x in turn], kbatch,
                                                 wrapped=wrapped, max_candidates=cap)
        t2 = time.perf_counter()
        # the chord walk for the points a run is short of: start rows and walk seed from the run's own generator
        short = []
        for j, (r, dead, lstar, alive) in enumerate(turn):
            nf = int(nfound[j])
            r.nclusters.append(int(ncl[j]))
            r.rcalls.append(int(ncalls[j]))
            r.eff.append(nf / int(ncalls[j]) if int(ncalls[j]) > 0 else float("nan"))
            r.ncall += int(ncalls[j])
            rows = dead[:nf]
            r.u[rows], r.theta[rows], r.logl[rows] = cu[j, :nf], ct[j, :nf], cl[j, :nf]
            if nf < kbatch:
                k = kbatch - nf
                start = alive[r.rng.integers(0, len(alive), k)]
                short.append((r, dead[nf:], lstar, _whitening(uas[j]), start, int(r.rng.integers(0, 2 ** 62))))
                r.fallbacks += k
        if short and walker_runs is not None:
            sizes = [len(rows) for _r, rows, *_x in short]
            wu, wt, wl, used = walker_runs(np.concatenate([r.u[st] for r, _rows, _l, _c, st, _s in short]),
                                           np.concatenate([r.theta[st] for r, _rows, _l, _c, st, _s in short]),
                                           np.concatenate([r.logl[st] for r, _rows, _l, _c, st, _s in short]),
                                           np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                                           np.array([t[2] for t in short], dtype=np.float64), np.stack([t[3] for t in short]),
                                           wrapped, nsteps, 200, [t[5] for t in short])
            a = 0
            for g, (r, rows, *_x) in enumerate(short):
                b = a + len(rows)
                r.u[rows], r.theta[rows], r.logl[rows] = wu[a:b], wt[a:b], wl[a:b]
                r.ncall += int(used[g]); r.fallback_calls += int(used[g])
                a = b
        else:
            for r, rows, lstar, chol, start, _wseed in short:
                wu, wt, wl = r.u[start], r.theta[start], r.logl[start]
                used = _host_chord_walk(wu, wt, wl, lstar, chol, wrapped, nsteps, r.rng, evaluate)
                r.u[rows], r.theta[rows], r.logl[rows] = wu, wt, wl
                r.ncall += used; r.fallback_calls += used
        t3 = time.perf_counter()
        for r, *_x in turn:
            if precision_criterion is not None:
                if _precision_stop(r.logz, r.logx, r.logl, precision_criterion):
                    r.done = True
            elif np.max(r.logl) + r.logx < r.logz + stop_gap:
                r.done = True
            r.timing["walk_s"] += t3 - t1
            r.timing["turns"] += 1
            r.timing["host_s"] += (t1 - t0) / len(turn)
    out = []
    for r in runs:
        logw_live = r.logx - np.log(nlive) + r.logl
        logz_final = np.logaddexp(r.logz, _logaddexp_many(logw_live))
        all_theta = np.vstack([a.reshape(-1, ndim) for a in r.dead_theta] + [r.theta])
        all_logl = np.concatenate(r.dead_logl + [r.logl])
        all_logw = np.concatenate(r.dead_logw + [logw_live]) - logz_final
        out.append(NestedResult(float(logz_final), float(np.sqrt(max(r.h, 0.0) / nlive)), r.it, r.ncall, float(r.h),
                                all_theta, all_logl, all_logw, r.timing, np.array(r.nclusters, dtype=np.int64), nlive=nlive,
                                kbatch=kbatch, logl_birth=np.concatenate(r.dead_birth + [r.birth]),
                                region_fallbacks=int(r.fallbacks), region_efficiency=np.array(r.eff, dtype=np.float64),
                                region_calls=np.array(r.rcalls, dtype=np.int64), region_fallback_calls=int(r.fallback_calls)))
    return out


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
    if adaptive_nsteps is not None and live is not None:
        _check_resident_adaptive(live, distances, live_chol)
        if clustering:
            _check_resident_clustering(live, clusterer, live_chol, nboot)
        return _ensemble_resident(live, ndim, [int(seed)], nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                  clustering=clustering, nboot=nboot, adaptive_nsteps=adaptive_nsteps, min_nsteps=min_nsteps,
                                  max_nsteps=max_nsteps, pk=pk, precision_criterion=precision_criterion)[0]
    if clustering and live is not None:
        _check_resident_clustering(live, clusterer, live_chol, nboot)
        return _ensemble_resident(live, ndim, [int(seed)], nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                  clustering=True, nboot=nboot, pk=pk, precision_criterion=precision_criterion)[0]
    if walker is not None and walker_runs is not None:
        raise ValueError("pass walker= or walker_runs=, not both")
    if clustering:
        clusterer = _default_clusterer(clusterer)
    nclusters = [] if clustering else None
    rng = np.random.default_rng(seed)
    defaults = ultranest_defaults(ndim)
    nlive = int(nlive or defaults["nlive"])
    kbatch = int(kbatch or max(1, nlive // 4))
    if not 1 <= kbatch < nlive:
        raise ValueError("need 1 <= kbatch < nlive")
    nsteps = int(nsteps or defaults["nsteps"])
    adapting = _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, distances)
    trace, fars = [], []
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool)
    u = rng.random((nlive, ndim))
    if live is not None:
        if live_chol not in ("device", "host"):
            raise ValueError(live_chol)
        theta = None
        logl = live.live_init(u)
        if live_chol == "device":
            u = None                                   # no host mirror of the rows at all
    else:
        theta = np.asarray(prior(u), dtype=np.float64)
        logl = np.asarray(loglike(theta), dtype=np.float64)
    ncall = nlive
    dead_theta, dead_logl, dead_logw = [], [], []
    birth, dead_birth = np.full(nlive, -np.inf), []      # (host order: every path but device_order, which reads them at the end)
    logz, h, logx = -np.inf, 0.0, 0.0
    it = 0
    # the resident live set with the ORDER on the device as well (GpuRVModel.live_sort, round 4): no per-point state on the host
    # at all — per iteration the log-L of the dying points comes down (the evidence sums need them), ranks go up
    device_order = live is not None and u is None and hasattr(live, "live_sort")
    top = float(np.max(logl)) if device_order else None
    # precision_criterion on the device-ordered path: the live log-L multiset, from the values that come down anyway
    live_ll = np.sort(logl) if device_order and precision_criterion is not None else None
    timing = {"order_s": 0.0, "step_wait_s": 0.0, "turns": 0}
    while it < max_iter and ncall < max_calls:
        timing["turns"] += 1
        t_turn = time.perf_counter()
        if device_order:
            dl, lstar, top = live.live_sort(kbatch)
            timing["order_s"] += time.perf_counter() - t_turn
            ranks = rng.integers(0, nlive - kbatch, kbatch)          # (the draw the host order's alive[rng.integers(...)] makes)
            seed_it = int(rng.integers(0, 2 ** 62))
            pending = _helper().submit(live.live_step, None, kbatch, ranks, lstar, wrapped, nsteps, 200, seed_it, **pk)
            order = dead = None
        else:
            order = _stable_argsort(logl)
            dead = order[:kbatch]
            lstar = logl[dead[-1]]
            dl = logl[dead]
            dead_birth.append(birth[dead])
            birth[dead] = lstar                                   # (the replacements of this iteration are drawn above lstar)
            timing["order_s"] += time.perf_counter() - t_turn
        if device_order:
            pass
        elif live is not None and u is None:
            # the resident live set, whitening on the device: the walk needs nothing of this iteration's evidence
            # bookkeeping, so it starts first — on a helper thread (the C call releases the interpreter lock) — and the
            # vectorised sums below run on the host while the GPU walks
            alive = order[kbatch:]
            start = alive[rng.integers(0, len(alive), kbatch)]
            seed_it = int(rng.integers(0, 2 ** 62))
            pending = _helper().submit(live.live_step, order, kbatch, start, lstar, wrapped, nsteps, 200, seed_it, **pk)
        else:
            pending = None
        logw, logz, h, logx = _deaths(logz, h, logx, dl, nlive, kbatch)
        if live is None:
            dead_theta.append(theta[dead])                                                # (index arrays: already copies)
        dead_logl.append(dl); dead_logw.append(logw)
        it += kbatch
        if pending is not None:
            t_wait = time.perf_counter()
            wl, used = pending.result()
            timing["step_wait_s"] += time.perf_counter() - t_wait
            ncall += int(used)
            if device_order:
                top = max(top, float(np.max(wl)))                     # the survivors' highest and the newcomers'
                if live_ll is not None:
                    live_ll = _multiset_step(live_ll, kbatch, wl)
            else:
                logl[dead] = wl
                top = np.max(logl)
            if precision_criterion is not None:
                if _precision_stop(logz, logx, live_ll if device_order else logl, precision_criterion):
                    break
            elif top + logx < logz + np.log(np.expm1(dlogz)):
                break
            continue
        alive = order[kbatch:]
        # whitening from the surviving live points
        chol = _whitening(u[alive]) if u is not None else None
        pick = rng.integers(0, len(alive), kbatch)
        start = alive[pick]
        if live is not None:
            # live_chol="host": order and start rows up, the new log-L of the replaced rows down, and the mirror of the rows
            wl, used = live.live_step(order, kbatch, start, lstar, wrapped, nsteps, 200, int(rng.integers(0, 2 ** 62)), chol=chol,
                                      **pk)
            ncall += int(used)
            logl[dead] = wl
            u = live.live_get()[0]
            if _stop(logz, logx, logl, dlogz, precision_criterion):
                break
            continue
        wu, wt, wl = u[start], theta[start], logl[start]
        starts = wu.copy() if adapting else None
        factors = [chol]
        cw = np.zeros(kbatch, dtype=np.intp)
        labels = None
        if clustering:
            ua = u[alive]
            labels, ncl, _ = clusterer(ua, [0, len(ua)], _cluster_scale(ua)[None, :], wrapped, nboot,
                                       [(int(seed) * _BOOT_MUL + it) & _M64])
            nclusters.append(int(ncl[0]))
            factors = _cluster_factors(ua, labels, int(ncl[0]), chol)
            cw = np.asarray(labels, dtype=np.intp)[pick]
        if walker is not None:
            wu, wt, wl, used = walker(wu, wt, wl, lstar, chol, wrapped, nsteps, 200, int(rng.integers(0, 2 ** 62)), **pk)
            ncall += int(used)
        elif walker_runs is not None:
            wo, sizes, gf, gseeds = _walk_groups(cw, factors, int(rng.integers(0, 2 ** 62)))
            gu, gt, gl, used = walker_runs(wu[wo], wt[wo], wl[wo], np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                                           np.full(len(sizes), lstar), np.stack(gf), wrapped, nsteps, 200, gseeds, **pk)
            wu[wo], wt[wo], wl[wo] = gu, gt, gl
            ncall += int(np.sum(used))
        many = len(factors) > 1
        if many:
            wfac = np.stack(factors)[cw]                        # each walker's factor: that of its start row's cluster
        if pk and walker is None and walker_runs is None:
            def evaluate(cand):
                if prior_loglike is not None:
                    return prior_loglike(cand)
                ct = np.asarray(prior(cand), dtype=np.float64)
                return ct, np.asarray(loglike(ct), dtype=np.float64)
            from .stepout import walk as stepout_walk
            ncall += stepout_walk(wu, wt, wl, lstar, wfac if many else chol, wrapped, nsteps, 200, pk["step_width"], rng, evaluate)
        for _ in range(0 if (walker is not None or walker_runs is not None or pk) else nsteps):
            z = rng.standard_normal((kbatch, ndim))
            d = np.einsum("kij,kj->ki", wfac, z) if many else z @ chol.T
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            tmin, tmax = _chord(wu, d, wrapped)
            todo = np.arange(kbatch)
            rounds = 0
            while todo.size and rounds < 200:
                t = tmin[todo] + (tmax[todo] - tmin[todo]) * rng.random(todo.size)
                cand = wu[todo] + t[:, None] * d[todo]
                if wrapped is not None:
                    cand[:, wrapped] %= 1.0
                cand = np.clip(cand, 0.0, np.nextafter(1.0, 0.0))
                if prior_loglike is not None:
                    ct, cl = prior_loglike(cand)                        # one round trip to the GPU
                else:
                    ct = np.asarray(prior(cand), dtype=np.float64)
                    cl = np.asarray(loglike(ct), dtype=np.float64)      # one batch = one GPU launch
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
        u[dead], theta[dead], logl[dead] = wu, wt, wl
        if adapting:
            from .adapt import far_fraction, next_nsteps
            c, f = _adapt_counts([(u[alive], None if labels is None else np.asarray(labels, dtype=np.intp), factors, cw, starts,
                                   wu)], adapting[2], wrapped)
            trace.append(nsteps)
            fars.append(float(far_fraction(f[0], c[0])))
            nsteps = next_nsteps(nsteps, int(f[0]), int(c[0]), adapting[0], adapting[1])
        if _stop(logz, logx, logl, dlogz, precision_criterion):
            break
    if device_order:
        logl = live.live_get(cube=False, theta=False)[2]              # the live points' log-L: once, at the end
    logw_live = logx - np.log(nlive) + logl
    logz_final = np.logaddexp(logz, _logaddexp_many(logw_live))
    if live is not None and hasattr(live, "live_dead_count"):
        # the samples come down once, straight into the array that is returned: dead points first, then the live set
        ndead = live.live_dead_count()
        all_theta = np.empty((ndead + nlive, ndim))
        live.live_dead(theta_out=all_theta[:ndead])
        live.live_get(cube=False, logl=False, theta_out=all_theta[ndead:])
    else:
        if live is not None:
            dead_theta = [live.live_dead()[0]]
            theta = live.live_get()[1]
        all_theta = np.vstack([a.reshape(-1, ndim) for a in dead_theta] + [theta])
    all_logl = np.concatenate(dead_logl + [logl])
    all_logw = np.concatenate(dead_logw + [logw_live]) - logz_final
    if live is not None and hasattr(live, "live_births"):
        all_birth = np.concatenate(live.live_births())        # the device's own record (it chose the dying rows)
    elif device_order:
        all_birth = None                                      # (a live set without births: the host never saw which rows died)
    else:
        all_birth = np.concatenate(dead_birth + [birth])
    return NestedResult(float(logz_final), float(np.sqrt(max(h, 0.0) / nlive)), it, ncall, float(h),
                        all_theta, all_logl, all_logw, timing, None if nclusters is None else np.array(nclusters, dtype=np.int64),
                        nlive=nlive, kbatch=kbatch, logl_birth=all_birth,
                        nsteps_trace=np.array(trace, dtype=np.int64) if adapting else None,
                        far_fraction=np.array(fars, dtype=np.float64) if adapting else None)


class _EnsembleRun:
    """One run of run_nested_ensemble: the state run_nested_slice keeps in its locals."""

    def __init__(self, seed, nlive, ndim):
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
        self.nclusters = []
        self.nsteps = None                          # adaptive_nsteps: this run's step count, its trace and far fractions
        self.trace, self.fars = [], []
        self.groups = None                          # adaptive_nsteps: (survivors, labels, factors, walker labels) of the turn


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
        _check_precision(precision_criterion)
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("need at least one seed")
        return _region_ensemble(prior, loglike, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped,
                                walker_runs, nboot, clusterer, region_runs, region_max_candidates, precision_criterion)
    pk = _walk_kwargs(proposal, step_width)
    _check_precision(precision_criterion)
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("need at least one seed")
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
    if clustering:
        clusterer = _default_clusterer(clusterer)
    defaults = ultranest_defaults(ndim)
    nlive = int(nlive or defaults["nlive"])
    kbatch = int(kbatch or max(1, nlive // 4))
    if not 1 <= kbatch < nlive:
        raise ValueError("need 1 <= kbatch < nlive")
    nsteps = int(nsteps or defaults["nsteps"])
    adapting = _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, distances)
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool)
    runs = [_EnsembleRun(s, nlive, ndim) for s in seeds]
    for r in runs:
        r.nsteps = nsteps
    theta = np.asarray(prior(np.concatenate([r.u for r in runs])), dtype=np.float64)
    logl = np.asarray(loglike(theta), dtype=np.float64)
    for i, r in enumerate(runs):
        r.theta, r.logl = theta[i * nlive:(i + 1) * nlive].copy(), logl[i * nlive:(i + 1) * nlive].copy()
    stop_gap = np.log(np.expm1(dlogz))
    while True:
        turn = []                                   # (run, dead rows, start rows, lstar, chol, walk seed)
        for r in runs:
            if r.done:
                continue
            if not (r.it < max_iter and r.ncall < max_calls):
                r.done = True
                continue
            t0 = time.perf_counter()
            order = _stable_argsort(r.logl)
            dead = order[:kbatch]
            lstar = r.logl[dead[-1]]
            dl = r.logl[dead]
            logw, r.logz, r.h, r.logx = _deaths(r.logz, r.h, r.logx, dl, nlive, kbatch)
            r.dead_theta.append(r.theta[dead])
            r.dead_logl.append(dl); r.dead_logw.append(logw)
            r.dead_birth.append(r.birth[dead])
            r.birth[dead] = lstar
            r.it += kbatch
            alive = order[kbatch:]
            chol = _whitening(r.u[alive])
            pick = r.rng.integers(0, len(alive), kbatch)
            start = alive[pick]
            turn.append((r, dead, start, lstar, chol, int(r.rng.integers(0, 2 ** 62)), alive, pick))
            r.timing["host_s"] += time.perf_counter() - t0
        if not turn:
            break
        if adapting:
            starts = [r.u[st] for r, _d, st, *_x in turn]
        if clustering:
            turn = _cluster_turn(turn, clusterer, wrapped, nboot, keep_groups=bool(adapting))
        else:
            if adapting:
                for r, _d, _st, _ls, chol, _sd, alive, _pick in turn:
                    r.groups = (r.u[alive], None, [chol], np.zeros(kbatch, dtype=np.intp))
            turn = [t[:6] + (np.arange(kbatch), [kbatch], [t[4]], [t[5]]) for t in turn]
        # (run, dead rows, start rows, lstar, chol, walk seed, walker order, group sizes, group factors, group seeds)
        sizes = np.concatenate([t[7] for t in turn])
        run_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        steps = nsteps
        if adapting:
            steps = np.repeat([t[0].nsteps for t in turn], [len(t[7]) for t in turn]).astype(np.int32)
            steps = int(steps[0]) if np.all(steps == steps[0]) else steps
        t0 = time.perf_counter()
        wu, wt, wl, used = walker_runs(np.concatenate([r.u[st[wo]] for r, _, st, _, _, _, wo, *_ in turn]),
                                       np.concatenate([r.theta[st[wo]] for r, _, st, _, _, _, wo, *_ in turn]),
                                       np.concatenate([r.logl[st[wo]] for r, _, st, _, _, _, wo, *_ in turn]),
                                       run_start, np.repeat([t[3] for t in turn], [len(t[7]) for t in turn]),
                                       np.stack([f for t in turn for f in t[8]]),
                                       wrapped, steps, 200, [s for t in turn for s in t[9]], **pk)
        t_walk = time.perf_counter() - t0
        g = 0
        for j, (r, dead, _st, _ls, _ch, _sd, wo, gsizes, *_rest) in enumerate(turn):
            t0 = time.perf_counter()
            rows = slice(j * kbatch, (j + 1) * kbatch)
            r.ncall += int(np.sum(used[g:g + len(gsizes)]))
            g += len(gsizes)
            back = dead[wo]                                  # the walkers' rows in group order
            r.u[back], r.theta[back], r.logl[back] = wu[rows], wt[rows], wl[rows]
            if precision_criterion is not None:
                if _precision_stop(r.logz, r.logx, r.logl, precision_criterion):
                    r.done = True
            elif np.max(r.logl) + r.logx < r.logz + stop_gap:
                r.done = True
            r.timing["walk_s"] += t_walk
            r.timing["turns"] += 1
            r.timing["host_s"] += time.perf_counter() - t0
        if adapting:
            from .adapt import far_fraction, next_nsteps
            t0 = time.perf_counter()
            c, f = _adapt_counts([t[0].groups + (starts[j], t[0].u[t[1]]) for j, t in enumerate(turn)], adapting[2], wrapped)
            dt = (time.perf_counter() - t0) / len(turn)
            for j, t in enumerate(turn):
                r = t[0]
                r.trace.append(r.nsteps)
                r.fars.append(float(far_fraction(f[j], c[j])))
                r.nsteps = next_nsteps(r.nsteps, int(f[j]), int(c[j]), adapting[0], adapting[1])
                r.groups = None
                r.timing["host_s"] += dt
    out = []
    for r in runs:
        logw_live = r.logx - np.log(nlive) + r.logl
        logz_final = np.logaddexp(r.logz, _logaddexp_many(logw_live))
        all_theta = np.vstack([a.reshape(-1, ndim) for a in r.dead_theta] + [r.theta])
        all_logl = np.concatenate(r.dead_logl + [r.logl])
        all_logw = np.concatenate(r.dead_logw + [logw_live]) - logz_final
        out.append(NestedResult(float(logz_final), float(np.sqrt(max(r.h, 0.0) / nlive)), r.it, r.ncall, float(r.h),
                                all_theta, all_logl, all_logw, r.timing,
                                np.array(r.nclusters, dtype=np.int64) if clustering else None, nlive=nlive, kbatch=kbatch,
                                logl_birth=np.concatenate(r.dead_birth + [r.birth]),
                                nsteps_trace=np.array(r.trace, dtype=np.int64) if adapting else None,
                                far_fraction=np.array(r.fars, dtype=np.float64) if adapting else None))
    return out


def _cluster_turn(turn, clusterer, wrapped, nboot, keep_groups=False):
    """run_nested_ensemble(clustering=True): the survivors of every run of the turn clustered in ONE clusterer call, then per
    run its walkers grouped by cluster as run_nested_slice groups them.  Appends the group order, sizes, factors and seeds
    to every turn entry; keep_groups: leaves (survivors, labels, factors, walker labels) in every run's `groups`."""
    t0 = time.perf_counter()
    uas = [r.u[alive] for r, *_x, alive, _pick in turn]
    run_start = np.concatenate([[0], np.cumsum([len(ua) for ua in uas])]).astype(np.int64)
    labels, ncl, _ = clusterer(np.concatenate(uas), run_start, np.stack([_cluster_scale(ua) for ua in uas]), wrapped, nboot,
                               [(r.seed * _BOOT_MUL + r.it) & _M64 for r, *_x in turn])
    labels = np.asarray(labels, dtype=np.intp)
    dt = (time.perf_counter() - t0) / len(turn)
    out = []
    for j, (r, dead, start, lstar, chol, wseed, alive, pick) in enumerate(turn):
        t0 = time.perf_counter()
        lab = labels[run_start[j]:run_start[j + 1]]
        r.nclusters.append(int(ncl[j]))
        factors = _cluster_factors(uas[j], lab, int(ncl[j]), chol)
        wo, sizes, gf, gseeds = _walk_groups(lab[pick], factors, wseed)
        if keep_groups:
            r.groups = (uas[j], lab, factors, lab[pick])
        out.append((r, dead, start, lstar, chol, wseed, wo, sizes, gf, gseeds))
        r.timing["host_s"] += dt + time.perf_counter() - t0
    return out


def _ensemble_resident(live, ndim, seeds, nlive, kbatch, nsteps, dlogz, max_iter, max_calls, wrapped, clustering=False, nboot=30,
                       adaptive_nsteps=None, min_nsteps=None, max_nsteps=None, pk=None, precision_criterion=None):
    """run_nested_ensemble(live=model): the device_order branch of run_nested_slice for every seed, the runs' live sets resident
    side by side (run r = rows r nlive .. r nlive + nlive - 1 of the ensemble), their bookkeeping vectorised across runs.
    clustering: the clustered step, with run r's bootstrap seed (seeds[r] _BOOT_MUL + deaths after this iteration) mod 2^64 —
    what run_nested_slice's host clustered path passes.  adaptive_nsteps: every run walks with its own step count, and the step
    returns the walkers' distances from the device rows (GpuRVModel.live_runs_step(nsteps=[...], return_distances=True))."""
    defaults = ultranest_defaults(ndim)
    nlive = int(nlive or defaults["nlive"])
    kbatch = int(kbatch or max(1, nlive // 4))
    if not 1 <= kbatch < nlive:
        raise ValueError("need 1 <= kbatch < nlive")
    nsteps = int(nsteps or defaults["nsteps"])
    adapting = _adapt_setup(adaptive_nsteps, nsteps, min_nsteps, max_nsteps, None)
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool)
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
        logw_live = logx_run[r] - np.log(nlive) + logl
        logz_final = np.logaddexp(logz[r], _logaddexp_many(logw_live))
        ndead = live.live_runs_dead_count(r)
        all_theta = np.empty((ndead + nlive, ndim))
        live.live_runs_dead(r, theta_out=all_theta[:ndead])
        live.live_runs_get(r, cube=False, logl=False, theta_out=all_theta[ndead:])
        all_logl = np.concatenate(dead_logl[r] + [logl])
        all_logw = np.concatenate(dead_logw[r] + [logw_live]) - logz_final
        all_birth = np.concatenate(live.live_runs_births(r)) if hasattr(live, "live_runs_births") else None
        out.append(NestedResult(float(logz_final), float(np.sqrt(max(h[r], 0.0) / nlive)), int(niter[r]), int(ncall[r]), float(h[r]),
                                all_theta, all_logl, all_logw, timing[r],
                                np.array(ncls[r], dtype=np.int64) if clustering else None, nlive=nlive, kbatch=kbatch,
                                logl_birth=all_birth,
                                nsteps_trace=np.array(trace[r], dtype=np.int64) if adapting else None,
                                far_fraction=np.array(fars[r], dtype=np.float64) if adapting else None))
    return out
