"""Posterior-predictive RV curves of merged nested-sampling runs with run-to-run error bars: the phase folds that the reference's
post_processing.py plots (the data folded on a planet's period with the other planets, the offsets, the drift and the linear
terms taken out, and the planet's curve on top), as numbers, and around the curve the band of the posterior with its scatter over
the replicates of the merged run.  DESIGN §4o.

The band comes from equal-weight draws (draws.py): n draws a replicate, their curves at the requested times, and per time the
order statistics of the n curve values — 1.3·10^8 curve values at 1000 replicates, 256 draws and 512 times, where a weighted band
over every row of every replicate would take 1.3·10^12.

    bands_definition   per group of n curves and per time: the values that are not NaN, sorted ascending; n_valid their number;
                       q[k] = sorted[max(0, ceil(level_k · n_valid) - 1)], the product taken in float64 (the inverted CDF of equal
                       weights, posterior.py's convention); mean = the left-to-right sum of the sorted values (np.cumsum's
                       order) over n_valid; NaN where n_valid = 0.  GpuRVModel.kep_rv_bands (rvll_kep_rv_bands;
                       csrc/rvll_bands.hip) reproduces it bit for bit on the curves of kep_rv_batch / modelk_batch.
"""
import numpy as np

from . import draws, posterior

MAX_GROUP = 4096
MAX_LEVELS = 16
QUANTILES = (0.15865, 0.5, 0.84135)


def check_levels(levels):
    """levels as float64 [Q]; raises ValueError where rvll_kep_rv_bands returns RVLL_E_INVALID for them."""
    levels = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
    if not 1 <= levels.shape[0] <= MAX_LEVELS:
        raise ValueError(f"need 1 to {MAX_LEVELS} quantile levels, got {levels.shape[0]}")
    if not np.all((levels > 0.0) & (levels < 1.0)):
        raise ValueError("quantile levels must lie in the open interval (0, 1)")
    return levels


def bands_definition(values, levels):
    """values float64 [G, n, T] (n <= 4096; NaN: an invalid orbit), levels [Q] in (0, 1): (q [G, Q, T], mean [G, T], n_valid
    int32 [G, T]) by the module's definition."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("values must be [groups, n, times]")
    if not 1 <= values.shape[1] <= MAX_GROUP:
        raise ValueError(f"a group holds 1 to {MAX_GROUP} rows")
    levels = check_levels(levels)
    G, n, T = values.shape
    srt = np.sort(values, axis=1)                                         # NaN last
    nv = np.count_nonzero(~np.isnan(values), axis=1).astype(np.int32)    # [G, T]
    q = np.full((G, levels.shape[0], T), np.nan)
    mean = np.full((G, T), np.nan)
    some = nv > 0
    for k, lv in enumerate(levels):
        idx = np.maximum(np.ceil(lv * nv.astype(np.float64)).astype(np.int64) - 1, 0)
        pick = np.take_along_axis(srt, np.minimum(idx, n - 1)[:, None, :], axis=1)[:, 0, :]
        q[:, k, :] = np.where(some, pick, np.nan)
    csum = np.cumsum(np.where(np.isnan(srt), 0.0, srt), axis=1)           # sequential, left to right; the NaN tail adds +0.0
    last = np.take_along_axis(csum, np.maximum(nv.astype(np.int64) - 1, 0)[:, None, :], axis=1)[:, 0, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(some, last / nv, np.nan)
    return q, mean, nv


def _over_replicates(x, alive):
    """mean, std (ddof 0), min, max of x [S, ...] over the replicates with alive[s] (at least one)."""
    x = x[alive]
    return x.mean(axis=0), x.std(axis=0), x.min(axis=0), x.max(axis=0)


def curve_bands(results, model, times, planet=None, exclude_planet=None, ndraws=256, nsamples=200, quantiles=QUANTILES, seed=0,
                mode="random", bootstrap=True, device=0, return_replicates=False):
    """The posterior band of a Keplerian curve at `times` from finished runs (a list of NestedResult with samples and
    logl_birth) of `model` (a GpuRVModel): the curve of `planet` alone (modelk) or, with planet=None, of all planets except
    exclude_planet (kep_rv).  Every replicate of the merged run (merge.py: mode / bootstrap / seed) gives ndraws equal-weight
    draws (draws.samples), their curves give per time the quantiles `quantiles` and the mean (bands_definition), and the
    replicates that have draws give per (level, time) the statistics of those.  A dict: band [Q, T] (the mean over the
    replicates), band_err (their standard deviation, ddof 0), band_min, band_max, mean, mean_err [T] (the same for the mean
    curve), n_valid_min [T] (the fewest valid curves a replicate had at that time), replicates (how many had draws), times and
    quantiles; with return_replicates also q [S, Q, T], mean_replicates [S, T] and alive [S] (the replicates that had draws).

    band_err holds the run-to-run scatter (with bootstrap=True: the bootstrap of the runs on top of the simulated shrinkage).
    It also holds the resampling noise of drawing ndraws rows a replicate, which falls as 1 / sqrt(ndraws): compare two values
    of ndraws before reading a small band_err as the runs' agreement.

    device=k draws on device k and reduces the curves where model writes them (model.kep_rv_bands); device=None runs the two
    numpy definitions on the curves that model.kep_rv_batch / modelk_batch return."""
    times = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
    levels = check_levels(quantiles)
    theta = draws.samples(results, ndraws, nsamples, seed, mode, bootstrap, device)          # [S, n, ndim]
    alive = ~np.isnan(theta[:, 0, 0])
    if not alive.any():
        raise ValueError("no replicate of the merged run has weight: nothing to draw from")
    # a replicate without draws is left out below; until then it stands in with the first live replicate's rows
    theta = np.where(alive[:, None, None], theta, theta[int(np.argmax(alive))][None])
    if device is None:
        flat = theta.reshape(-1, theta.shape[2])
        curves = model.modelk_batch(flat, times, planet) if planet is not None else model.kep_rv_batch(flat, times, exclude_planet)
        q, mean, nv = bands_definition(curves.reshape(theta.shape[0], theta.shape[1], times.shape[0]), levels)
    else:
        q, mean, nv = model.kep_rv_bands(theta, times, levels, planet=planet, exclude_planet=exclude_planet)
    band, band_err, band_min, band_max = _over_replicates(q, alive)
    mean_, mean_err, _, _ = _over_replicates(mean, alive)
    n_valid_min = nv[alive].min(axis=0)
    out = dict(band=band, band_err=band_err, band_min=band_min, band_max=band_max, mean=mean_, mean_err=mean_err,
               n_valid_min=n_valid_min, replicates=int(alive.sum()), times=times, quantiles=levels)
    if return_replicates:
        out.update(q=q, mean_replicates=mean, alive=alive)
    return out


def gp_bands(gp, thetas, times, quantiles=QUANTILES, return_var=True):
    """The band of a correlated-noise model's GP over posterior draws: gp a correlated.CorrelatedNoiseModel, thetas [n, ndim]
    (n <= 4096) what draws.samples returns for one replicate, times [T].  Every row's conditional mean at `times` comes from
    gp.predict_batch on the device; per time the quantiles `quantiles` and the mean of those n means over the rows
    (bands_definition, on the host; a row without a valid orbit or covariance is NaN and is left out).  With return_var also
    total_sd [T] = sqrt(mean over the rows of var + variance over the rows of the mean, ddof 0): the GP's own uncertainty and the
    posterior's spread of its mean together; it costs the O(T Ne J) a row of predict_batch's return_var.  A dict: band [Q, T],
    mean [T], n_valid [T], total_sd [T] (None without return_var), times and quantiles."""
    times = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
    levels = check_levels(quantiles)
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim != 2:
        raise ValueError("thetas must be [draws, ndim]: one replicate of draws.samples")
    pred = gp.predict_batch(thetas, times, return_var=return_var)
    q, mean, nv = bands_definition(pred.mean[None], levels)
    total_sd = None
    if return_var:
        ok = ~np.isnan(pred.mean)
        cnt = np.maximum(ok.sum(axis=0), 1)
        m = np.where(ok, pred.mean, 0.0).sum(axis=0) / cnt
        spread = np.where(ok, (pred.mean - m) ** 2, 0.0).sum(axis=0) / cnt
        own = np.where(ok, pred.var, 0.0).sum(axis=0) / cnt
        total_sd = np.where(ok.any(axis=0), np.sqrt(np.maximum(own + spread, 0.0)), np.nan)
    return dict(band=q[0], mean=mean[0], n_valid=nv[0], total_sd=total_sd, times=times, quantiles=levels)


def _slot(spec, theta):
    return float(theta[spec.index]) if spec.is_free else float(spec.value)


def phase_fold_data(model, theta, planet):
    """The points of the reference's phase-fold plot of `planet` (1-based) for one parameter vector theta [ndim]
    (post_processing.py:396-444), as numbers.  A dict with, per epoch in the order of model.table: phase (days, in
    [-period / 2, period / 2)), rv — the datum with the instrument's offset, the curve of the other planets
    (kep_rv(exclude_planet=planet)), the drift and the linear terms taken out —, rv_err (the datum's error with the instrument's
    jitter in quadrature when jitter is in the model), inst (the instrument index) and model (the planet's own curve at the
    epoch); and t_ref and period.  As in the reference: the drift of an instrument's epochs is taken about the first of *those*
    epochs unless drift_tref is a parameter, and t_ref is the epoch of the first instrument at which the planet's curve is
    largest — or, while that epoch is exactly 0, of the next instrument (`if t_ref == 0`).  model: a GpuRVModel, or any object
    with its layout, table, linpar_dict, kep_rv_batch and modelk_batch."""
    lay, tab = model.layout, model.table
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    if theta.shape[0] != lay.ndim:
        raise ValueError(f"expected {lay.ndim} parameters, got {theta.shape[0]}")
    if not 1 <= int(planet) <= lay.nplanets:
        raise KeyError(f"planet{planet}_period")
    spec = lay.planets[int(planet) - 1]
    praw = _slot(spec.p, theta)
    period = float(np.exp(praw)) if spec.p_kind else praw                 # P_LOGPERIOD = 1
    time, ne = tab.time, tab.time.shape[0]
    others = model.kep_rv_batch(theta[None, :], time, exclude_planet=int(planet))[0]
    own = model.modelk_batch(theta[None, :], time, int(planet))[0]
    phase, rv, err = np.zeros(ne), np.zeros(ne), np.zeros(ne)
    t_ref = 0
    for i, inst in enumerate(lay.insts):
        idx = np.where(tab.inst_id == i)
        t = time[idx]
        corrected = tab.vrad[idx] - _slot(inst.offset, theta)
        corrected -= others[idx]
        if lay.has_drift:
            lin, quad, cub, quar = (_slot(s, theta) for s in lay.drift)
            tref = t[0] if lay.tref_from_data else _slot(lay.tref, theta)
            tt = (t - tref) / 365.25
            corrected -= lin * tt + quad * tt ** 2 + cub * tt ** 3 + quar * tt ** 4
        if lay.has_linpar:
            for name, s in zip(lay.linpar_names, lay.linpar):
                corrected -= _slot(s, theta) * np.asarray(model.linpar_dict[name], dtype=np.float64)[idx]
        yerr = tab.svrad[idx]
        err[idx] = np.sqrt(yerr ** 2 + _slot(inst.jitter, theta) ** 2) if lay.has_jitter else yerr
        if t_ref == 0:
            t_ref = t[np.argmax(own[idx])]
        phase[idx] = (((t - t_ref) / period) % 1. - 0.5) * period
        rv[idx] = corrected
    return dict(phase=phase, rv=rv, rv_err=err, inst=np.asarray(tab.inst_id).copy(), model=own, t_ref=float(t_ref), period=period)


def phase_fold(results, model, parnames, planet, nphase=200, **kw):
    """The phase fold of `planet` with its band: phase_fold_data at the merged run's posterior mean (the Mean column of the
    reference's table, posterior.table's mean) and curve_bands(planet=planet) at t_ref + phase for nphase phases over one
    period, from -period / 2 to period / 2.  A dict: data (phase_fold_data's), phase [nphase], and curve_bands' entries.  kw:
    curve_bands' keywords (ndraws, nsamples, quantiles, seed, mode, bootstrap, device)."""
    device = kw.get("device", 0)
    tab = posterior.table(results, parnames, nsamples=1, seed=kw.get("seed", 0), mode="expected", bootstrap=False, device=device)
    theta = np.asarray(tab["mean"], dtype=np.float64)
    data = phase_fold_data(model, theta, planet)
    phase = np.linspace(-0.5, 0.5, int(nphase)) * data["period"]
    out = curve_bands(results, model, data["t_ref"] + phase, planet=planet, **kw)
    out.update(data=data, phase=phase, theta=theta)
    return out
