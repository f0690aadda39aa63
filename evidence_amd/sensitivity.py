"""Prior sensitivity of ln Z and p(k | y) from finished runs, without new sampling.

The merged run's weighted rows are draws from the posterior under the base prior pi.  For another prior pi' whose support lies
inside pi's,
    Z' / Z = E_posterior[ pi'(theta) / pi(theta) ],
and the rows reweighted by r = pi' / pi give every downstream quantity under pi' (Skilling 2006, "Nested sampling for general
Bayesian computation", §7; Chopin & Robert 2010).  With the table of pointwise.pointwise_arrays set to t = ln r, its lpd is
ln(sum p r / P) = ln(Z' / Z) per replicate of the merged run, so the replicate reduction is rvll_pointwise_replicates' fp64
product on the matrix units; the new device work is the table itself, rvll_prior_logpdf_batch (csrc/rvll_prior_density.hip),
whose numpy definition is priors.log_density.

Table.  [ln r, 2 ln r]: 2 A units for A alternatives.  A row that pi' excludes (ln r = -inf) enters as OUTSIDE = -1e29 (the
pointwise table takes |t| <= 1e30, and exp of it is 0).  Per replicate s and alternative a
    dlogz[s, a]      = lpd[s, a]                          = ln(sum p r / P)
    logz_new[s, a]   = logz[s] + dlogz[s, a]
    efficiency[s, a] = exp(2 lpd[s, a] - lpd[s, A + a])   = (sum p r)^2 / (P sum p r^2), in (0, 1]
the last the Kish size of the reweighted rows over that of the rows themselves: near 1 the alternative barely moves the
posterior, near 0 a few rows carry the estimate and dlogz is not to be trusted.  r is capped at its largest value over the rows
with weight (logwt >= -43 in the expected-weight run): that is the pointwise min(t - c, 0), which only touches rows without
weight.  An alternative that leaves no row with weight has dlogz = -inf and efficiency 0.  Pareto smoothing of the ratios is not
done; efficiency and outside are the diagnostics.
"""
import numpy as np

from . import _abi, fip, merge, pointwise, priors

OUTSIDE = -1e29                          # ln r of a row the alternative excludes, as the table carries it
MAX_LOGRATIO = 2.5e28                    # the largest finite |ln r|: twice it stays apart from OUTSIDE
MAX_SETS = 4096                        # sets of one device call (rvll_prior_logpdf_batch)
_SORTED = (_abi.DENSITY_SORTED_UNIFORM, _abi.DENSITY_SORTED_LOGUNIFORM)


def log_prior_sets(sets, thetas, device=None, timing=None):
    """float64 [N, A]: the log prior density of every row of thetas [N, ndim] under every set of sets (A lists of ndim PriorSpec;
    None: a parameter the set leaves out, RVLL_DENSITY_SKIP), each the sum over the parameters in rising order.  device=None
    evaluates the numpy definition (priors.log_density); device=k runs rvll_prior_logpdf_batch on device k (timing: a dict that
    receives the summed rvll_density_timing of the calls)."""
    thetas = np.ascontiguousarray(np.atleast_2d(np.asarray(thetas, dtype=np.float64)))
    sets = [list(s) for s in sets]
    n, ndim = thetas.shape
    if not sets or any(len(s) != ndim for s in sets):
        raise ValueError(f"need at least one set, each with one entry for every of the {ndim} parameters")
    out = np.empty((n, len(sets)))
    if device is None:
        for a, specs in enumerate(sets):
            out[:, a] = priors.log_density(specs, thetas)
        return out
    lib = _abi.load()
    total = dict(kernel_ms=0.0, total_ms=0.0, rows=n, elements=0, launches=0, threads=0)
    for a0 in range(0, len(sets), MAX_SETS):
        block = sets[a0:a0 + MAX_SETS]
        arr = (_abi.PriorDensity * (len(block) * ndim))()
        for a, specs in enumerate(block):
            for d, spec in enumerate(specs):
                priors.density_to_c(spec, arr[a * ndim + d])
        part = np.empty((n, len(block)))
        t = _abi.DensityTiming()
        _abi.check(lib.rvll_prior_logpdf_batch(int(device), arr, len(block), ndim, _abi.as_dp(thetas), n, _abi.as_dp(part),
                                               _abi.C.byref(t)))
        out[:, a0:a0 + len(block)] = part
        for key in ("kernel_ms", "total_ms", "elements", "launches"):
            total[key] += getattr(t, key)
        total["threads"] = t.threads
    if timing is not None:
        timing.update(total)
    return out


def _check_ratio(logratio, logl):
    logratio = np.asarray(logratio, dtype=np.float64)
    if logratio.ndim == 1:
        logratio = logratio[:, None]
    if logratio.ndim != 2 or logratio.shape[1] < 1 or logratio.shape[0] != np.asarray(logl).reshape(-1).shape[0]:
        raise ValueError("logratio must be [rows, alternatives] with one row for every row of logl")
    if np.isnan(logratio).any() or np.any(logratio == np.inf):
        raise ValueError("logratio must be finite or -inf: the base prior has to be above zero wherever rows were drawn")
    if np.any(np.abs(logratio[np.isfinite(logratio)]) > MAX_LOGRATIO):
        raise ValueError(f"a finite logratio is beyond {MAX_LOGRATIO} in size")
    return logratio


def _table(logratio):
    t = np.where(np.isneginf(logratio), OUTSIDE, logratio)
    return np.ascontiguousarray(np.concatenate([t, np.where(np.isneginf(logratio), OUTSIDE, 2.0 * t)], axis=1))


def _outside(logratio, logl, birth, run_start):
    """(outside [A], the number of rows with weight) on the expected-weight merged run."""
    m = merge.merge_arrays(logl, birth, run_start)
    rows = m["order"][m["logwt"] >= pointwise.WEIGHT_FLOOR]
    return np.count_nonzero(np.isneginf(logratio[rows]), axis=0).astype(np.int64), int(rows.shape[0])


def _reweight(logratio, table, pre, outside, logl, birth, run_start, nsamples, code, seed, bootstrap, device, block_bytes, timing):
    A = logratio.shape[1]
    out = pointwise._arrays(table, pre, logl, birth, run_start, nsamples, code, seed, bootstrap, device, block_bytes, None, timing)
    lpd = out["lpd"]
    dlogz = lpd[:, :A].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        eff = np.exp(2.0 * lpd[:, :A] - lpd[:, A:])
    dead = outside[0] == outside[1]                                   # no row with weight is left: Z' = 0 as far as the runs can say
    dlogz[:, dead] = -np.inf
    eff[:, dead] = 0.0
    return dict(dlogz=dlogz, logz_new=out["logz"][:, None] + dlogz, efficiency=eff, logz=out["logz"], information=out["information"],
                outside=outside[0])


def reweight_arrays(logratio, logl, birth, run_start, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None,
                    block_bytes=None, timing=None):
    """ln(Z' / Z) of A alternative priors over nsamples replicates of the merged run of the runs (logl, birth, run_start) as
    merge.replicates_arrays takes them.  logratio [N, A] in input row order: ln(pi'(theta) / pi(theta)) of every row, finite or
    -inf where pi' excludes the row.  A dict with dlogz, logz_new and efficiency [S, A] (module docstring); outside int64 [A],
    the rows of the expected-weight run with weight (logwt >= -43) that the alternative excludes; logz and information [S], the
    bits of merge.replicates_arrays.  r is capped at its largest value over the rows with weight (the pointwise min(t - c, 0)):
    a row without weight counts with at most that ratio.  An alternative that excludes every row with weight has dlogz = -inf
    and efficiency 0 in every replicate: Z' = 0 as far as the runs can say.  device=None: the numpy definition; device=k: the
    table is reduced by rvll_pointwise_replicates on device k (block_bytes, timing: pointwise.pointwise_arrays')."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    logratio = _check_ratio(logratio, logl)
    table = pointwise.check_table(_table(logratio), logl)
    pre = pointwise.shifts_of(table, logl, birth, run_start)
    return _reweight(logratio, table, pre, _outside(logratio, logl, birth, run_start), logl, birth, run_start, nsamples, code, seed,
                     bootstrap, device, block_bytes, timing)


def _group_of(parnames, priordict, name):
    """The parameters of the sorted group `name` belongs to under priordict (empty when its prior is not a sorted one)."""
    spec = priordict[name]
    if spec.density is None or spec.density[0] not in _SORTED:
        return []
    return [p for p in parnames if p in priordict and priordict[p].density is not None
            and priordict[p].density[0] == spec.density[0] and priordict[p].group == spec.group]


def alternative_sets(parnames, priordict, alternatives, skip_missing=False):
    """(base sets, alternative sets) for log_prior_sets: per alternative (a dict {parameter: PriorSpec} that overrides entries of
    priordict) one list over parnames with the base / the alternative spec at the overridden parameters and None elsewhere, so
    that identical factors never enter the ratio.  ValueError when an alternative names a parameter that is not free (with
    skip_missing those are left out: the alternative does not apply to this model), when its support is not inside the base
    prior's for that parameter (rows cannot carry mass where none were drawn), when it replaces a sorted prior by one that is
    not sorted, or overrides a sorted group only in part."""
    parnames = list(parnames)
    base_sets, alt_sets = [], []
    for i, alt in enumerate(alternatives):
        alt = dict(alt)
        for name in list(alt):
            if name not in parnames:
                if not skip_missing:
                    raise ValueError(f"alternative {i}: {name} is not a free parameter")
                del alt[name]
        for name, spec in alt.items():
            base = priordict[name]
            blo, bhi = priors.support(base)
            alo, ahi = priors.support(spec)
            if not (alo >= blo and ahi <= bhi):
                raise ValueError(f"alternative {i}: the support of {name}, [{alo}, {ahi}], is not inside the base prior's "
                                 f"[{blo}, {bhi}]")
            group = _group_of(parnames, priordict, name)
            if group:
                if spec.density[0] not in _SORTED:
                    raise ValueError(f"alternative {i}: {name} has a sorted base prior; the alternative must be sorted too")
                if any(p not in alt for p in group):
                    raise ValueError(f"alternative {i}: the sorted group of {name} is overridden only in part")
        base_sets.append([priordict[p] if p in alt else None for p in parnames])
        alt_sets.append([alt.get(p) for p in parnames])
    return base_sets, alt_sets


def log_ratios(samples, parnames, priordict, alternatives, device=None, skip_missing=False, timing=None):
    """float64 [N, A]: ln(pi'(theta) / pi(theta)) of every row of samples under every alternative, over the overridden
    parameters only (alternative_sets); -inf where the alternative excludes the row.  ValueError where the base prior itself
    is zero or NaN at a row."""
    base_sets, alt_sets = alternative_sets(parnames, priordict, alternatives, skip_missing)
    t0, t1 = {}, {}
    base = log_prior_sets(base_sets, samples, device, t0)
    new = log_prior_sets(alt_sets, samples, device, t1)
    if not np.isfinite(base).all():
        raise ValueError("the base prior is zero, infinite or NaN at some rows: they cannot have been drawn from it")
    if timing is not None and device is not None:
        timing.update({k: t0[k] + t1[k] for k in ("kernel_ms", "total_ms", "elements", "launches")})
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(new), -np.inf, new - base)


def prior_sensitivity(results, parnames, priordict, alternatives, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None,
                      block_bytes=None, skip_missing=False, timing=None):
    """ln Z under a list of alternative priors from finished runs (a list of NestedResult with samples and logl_birth, stacked as
    merge.merge stacks them) that were sampled under priordict, the priors of the free parameters parnames (the columns of the
    samples).  alternatives: a list of dicts {parameter name: PriorSpec} that override entries of priordict (alternative_sets
    says what is refused).  Returns a dict with, per alternative [A]: logz, dlogz and efficiency from the merged run's expected
    weights (mode="expected", no bootstrap, one replicate); logz_err, dlogz_err, dlogz_min, dlogz_max, the standard deviation
    and the range over nsamples replicates (mode / bootstrap / seed); outside, the rows with weight the alternative excludes;
    logz_base and logz_base_err, the same for the base prior; logratio [N, A]; nsamples; replicates, the reweight_arrays dict
    of the replicates.  device=None: the numpy definitions; device=k: rvll_prior_logpdf_batch and rvll_pointwise_replicates.
    timing: a dict that receives density (the table's rvll_density_timing, summed) and reduce (the replicates' pointwise
    timing)."""
    samples, logl, birth, run_start = pointwise._samples(results)
    if samples.shape[1] != len(list(parnames)):
        raise ValueError(f"the samples have {samples.shape[1]} columns, parnames {len(list(parnames))} names")
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    t_den, t_red = {}, {}
    logratio = _check_ratio(log_ratios(samples, parnames, priordict, alternatives, device, skip_missing, t_den), logl)
    table = pointwise.check_table(_table(logratio), logl)
    pre = pointwise.shifts_of(table, logl, birth, run_start)
    outside = _outside(logratio, logl, birth, run_start)
    point = _reweight(logratio, table, pre, outside, logl, birth, run_start, 1, _abi.SHRINK_EXPECTED, seed, False, device, block_bytes,
                      None)
    reps = _reweight(logratio, table, pre, outside, logl, birth, run_start, nsamples, code, seed, bootstrap, device, block_bytes, t_red)
    if timing is not None:
        timing.update(density=t_den, reduce=t_red)
    with np.errstate(invalid="ignore"):                               # an alternative without evidence (-inf) has no error: NaN
        logz_err, dlogz_err = np.std(reps["logz_new"], axis=0), np.std(reps["dlogz"], axis=0)
    return dict(logz=point["logz_new"][0], dlogz=point["dlogz"][0], efficiency=point["efficiency"][0], logz_err=logz_err,
                dlogz_err=dlogz_err, dlogz_min=np.min(reps["dlogz"], axis=0), dlogz_max=np.max(reps["dlogz"], axis=0),
                outside=reps["outside"], logz_base=float(point["logz"][0]), logz_base_err=float(np.std(reps["logz"])),
                logratio=logratio, nsamples=int(nsamples), replicates=reps)


def sensitivity_per_model(results_per_model, parnames_per_model, priordict_per_model, alternatives, seed=0, **kw):
    """prior_sensitivity of the models k = 0 .. K under one list of alternatives: model k is replicated with the seed
    fip.model_seed(seed, k), so that the bootstraps of different models are independent draws, as their runs are, and an
    alternative that names a parameter model k lacks does not apply there (its ratio is 1 over the rest).  The list
    model_probabilities takes."""
    return [prior_sensitivity(results_per_model[k], parnames_per_model[k], priordict_per_model[k], alternatives,
                              seed=fip.model_seed(seed, k), skip_missing=True, **kw) for k in range(len(results_per_model))]


def model_probabilities(sens_per_model):
    """p(k | y) under every alternative: sens_per_model[k] is the prior_sensitivity output of the model with k planets, k = 0 ..
    K, all for the same A alternatives and the same nsamples (sensitivity_per_model).  A dict with pky [K + 1, A], the softmax
    over k of the point values logz[k][a]; pky_err [K + 1, A], the standard deviation over the replicates s of the softmax over k
    of logz_new[k][s, a]; pky_replicates [S, K + 1, A]; logz [K + 1, A]."""
    sens = list(sens_per_model)
    if not sens:
        raise ValueError("need at least one model")
    shapes = {np.asarray(s["replicates"]["logz_new"]).shape for s in sens}
    if len(shapes) != 1:
        raise ValueError(f"the models' replicates differ in shape: {sorted(shapes)}")
    logz = np.stack([np.asarray(s["logz"], dtype=np.float64) for s in sens])                       # [K + 1, A]
    reps = np.stack([np.asarray(s["replicates"]["logz_new"], dtype=np.float64) for s in sens], axis=1)   # [S, K + 1, A]
    pky = fip._softmax(logz.T).T
    pky_s = np.swapaxes(fip._softmax(np.swapaxes(reps, 1, 2)), 1, 2)
    return dict(pky=pky, pky_err=np.std(pky_s, axis=0), pky_replicates=pky_s, logz=logz)
