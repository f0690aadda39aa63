"""Residual periodograms of merged nested-sampling runs with run-to-run error bars: the generalised Lomb-Scargle periodogram of
what the chosen model leaves of the data — the check that a k-planet model is adequate, and the classical counterpart of the FIP
periodogram — as a posterior band over equal-weight draws with its scatter over the replicates of the merged run.  DESIGN §4p.

    residuals_definition   `res` and `noise` of the reference's RVModel.log_likelihood (rvmodel/__init__.py:180-215) in numpy, in
                           the reference's order of additions: rvm = offset; rvm += kep_rv; rvm += drift; rvm += linpar terms;
                           res = vrad - rvm; var = svrad² (+ jitter²).  The drift is taken about drift_tref, or about time[0] of
                           the whole table (the likelihood's rule, not the phase fold's per-instrument one).  keep_planet=p leaves
                           planet p out of the subtraction.  An invalid orbit (a NaN curve) gives a NaN row of res.
                           GpuRVModel.residuals_batch (rvll_residuals_batch) is the device's.
    gls_definition         the GLS power with a floating mean (Zechmeister & Kürster 2009) per row on a uniform grid
                           f_k = f0 + df k with w = (1/var) / Σ(1/var), τ = time - min(time), φ = 2π f_k τ:
                               Y = Σ w r, C = Σ w cos φ, S = Σ w sin φ,
                               YY = Σ w r² - Y², YC = Σ w r cos φ - Y C, YS = Σ w r sin φ - Y S,
                               CC = Σ w cos² φ - C², SS = Σ w sin² φ - S², CS = Σ w cos φ sin φ - C S, D = CC SS - CS²,
                               p = (SS YC² + CC YS² - 2 CS YC YS) / (YY D),
                           NaN where YY D is not > 0 and for a NaN row.  GpuRVModel.gls_bands / gls_batch (rvll_gls_bands;
                           csrc/rvll_gls.hip) evaluate it on the device; tests/test_gpu_gls_windows.py holds them to this
                           definition in long double window by window of 512 frequencies, each row within 8 times the
                           float64 noise of its own window, on the default grid up to 2^18 + 3 frequencies.
                           Degenerate frequencies are not guarded: where every epoch has the same sine or cosine in exact
                           arithmetic (an evenly spaced table has such aliases of f = 0 and of half its sampling rate on
                           the default grid) CC, SS and D are rounding residue, and the power is NaN or a number without
                           meaning — in float64, in long double and on the device, each at its own entries.  The ratio
                           D / (CC SS) does not tell them apart (it is 1, -inf or NaN there, against 7e-5 at a sound
                           frequency of a 4-epoch table), so no threshold is applied; choose pmin above twice the spacing
                           of an evenly spaced table, and see peaks_definition for what a NaN does to the peaks.
"""
import numpy as np

from . import draws, predictive

MIN_EPOCHS = 4
MAX_FREQ = 1 << 24


def check_grid(f0, df, nfreq, nepochs=None):
    """(f0, df, nfreq) as (float, float, int); raises ValueError where rvll_gls_bands returns RVLL_E_INVALID for them."""
    f0, df = float(f0), float(df)
    if not (0.0 < f0 < np.inf and 0.0 < df < np.inf):
        raise ValueError("f0 and df must be positive and finite")
    if int(nfreq) != nfreq or not 1 <= int(nfreq) <= MAX_FREQ:
        raise ValueError(f"nfreq must be an integer in [1, {MAX_FREQ}]")
    if nepochs is not None and nepochs < MIN_EPOCHS:
        raise ValueError(f"a periodogram needs at least {MIN_EPOCHS} epochs")
    return f0, df, int(nfreq)


def frequency_grid(time, oversample=8, pmin=None):
    """(f0, df, nfreq) of the default grid over the epochs `time`: f0 = df = 1 / (oversample · span) up to 1 / pmin, where pmin
    defaults to twice the median spacing of the sorted epochs."""
    time = np.sort(np.asarray(time, dtype=np.float64).reshape(-1))
    if time.shape[0] < MIN_EPOCHS:
        raise ValueError(f"a periodogram needs at least {MIN_EPOCHS} epochs")
    span = float(time[-1] - time[0])
    if not span > 0.0:
        raise ValueError("the epochs span no time")
    if not float(oversample) > 0.0:
        raise ValueError("oversample must be positive")
    if pmin is None:
        pmin = 2.0 * float(np.median(np.diff(time)))
    if not (float(pmin) > 0.0 and np.isfinite(pmin)):
        raise ValueError("pmin must be positive and finite (the median spacing of the epochs is 0: pass pmin)")
    df = 1.0 / (float(oversample) * span)
    nfreq = max(1, int(np.floor(1.0 / (float(pmin) * df))))
    return check_grid(df, df, nfreq)


def _slot(spec, X):
    return X[:, spec.index] if spec.is_free else np.full(X.shape[0], float(spec.value))


def residuals_definition(model, theta, keep_planet=None):
    """(res [n, Ne], var [n, Ne]) of theta [n, ndim] (or [ndim]) by the module's definition.  model: a GpuRVModel, or any object
    with its layout, table, linpar_dict and kep_rv_batch (the duck type of predictive.phase_fold_data)."""
    lay, tab = model.layout, model.table
    X = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    if X.ndim != 2 or X.shape[1] != lay.ndim:
        raise ValueError(f"expected {lay.ndim} parameters a row, got {X.shape}")
    if not (keep_planet is None or type(keep_planet) is int):
        raise AssertionError(f"keep_planet has to be an {int}, got {type(keep_planet)}.")
    time = np.asarray(tab.time, dtype=np.float64)
    n, ne = X.shape[0], time.shape[0]
    rvm, var = np.zeros((n, ne)), np.zeros((n, ne))
    inst_id = np.asarray(tab.inst_id)
    for i, inst in enumerate(lay.insts):                                              # rvmodel:183-192
        idx = np.where(inst_id == i)[0]
        rvm[:, idx] += _slot(inst.offset, X)[:, None]
        if lay.has_jitter:
            var[:, idx] = (np.asarray(tab.svrad, dtype=np.float64)[idx] ** 2)[None, :] + (_slot(inst.jitter, X) ** 2)[:, None]
        else:
            var[:, idx] = (np.asarray(tab.svrad, dtype=np.float64)[idx] ** 2)[None, :]
    if lay.nplanets > 0:                                                              # rvmodel:195-203
        rvm += np.asarray(model.kep_rv_batch(X, time, exclude_planet=keep_planet), dtype=np.float64)
    if lay.has_drift:                                                                 # rvmodel:206-207, :242-271
        lin, quad, cub, quar = (_slot(s, X)[:, None] for s in lay.drift)
        tref = np.full((n, 1), time[0]) if lay.tref_from_data else _slot(lay.tref, X)[:, None]
        tt = (time[None, :] - tref) / 365.25
        rvm += lin * tt + quad * tt ** 2 + cub * tt ** 3 + quar * tt ** 4
    if lay.has_linpar:                                                                # rvmodel:210-212
        for name, s in zip(lay.linpar_names, lay.linpar):
            rvm += _slot(s, X)[:, None] * np.asarray(model.linpar_dict[name], dtype=np.float64)[None, :]
    res = np.asarray(tab.vrad, dtype=np.float64)[None, :] - rvm                       # rvmodel:215
    return res, var


def gls_definition(time, res, var, f0, df, nfreq, phase="f_tau", dtype=np.float64):
    """power [n, nfreq] of res, var [n, Ne] (or [Ne]) at the epochs `time` by the module's definition.  phase names the order
    in which φ = 2π f τ is multiplied out — "f_tau": (2π f) τ, "ftau": 2π (f τ), "tau_f": (2π τ) f — and dtype the arithmetic
    (np.longdouble: the yardstick of the device tests); the definition is the default of both."""
    f0, df, nfreq = check_grid(f0, df, nfreq)
    time = np.asarray(time, dtype=dtype).reshape(-1)
    res, var = np.atleast_2d(np.asarray(res, dtype=dtype)), np.atleast_2d(np.asarray(var, dtype=dtype))
    if res.shape != var.shape or res.ndim != 2 or res.shape[1] != time.shape[0]:
        raise ValueError("res and var must be [n, len(time)]")
    if time.shape[0] < MIN_EPOCHS:
        raise ValueError(f"a periodogram needs at least {MIN_EPOCHS} epochs")
    two_pi = dtype(2.0) * (np.pi if dtype is np.float64 else np.arccos(dtype(-1.0)))
    tau = time - time.min()
    f = dtype(f0) + dtype(df) * np.arange(nfreq, dtype=dtype)
    if phase == "f_tau":
        ph = (two_pi * f)[:, None] * tau[None, :]
    elif phase == "ftau":
        ph = two_pi * (f[:, None] * tau[None, :])
    elif phase == "tau_f":
        ph = (two_pi * tau)[None, :] * f[:, None]
    else:
        raise ValueError(f"unknown phase order {phase!r}")
    c, s = np.cos(ph), np.sin(ph)                                                     # [F, Ne]
    power = np.full((res.shape[0], nfreq), np.nan, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(res.shape[0]):
            inv = dtype(1.0) / var[b]
            w = inv / inv.sum()
            r = res[b]
            wr = w * r
            Y = wr.sum()
            C, S = (w * c).sum(axis=1), (w * s).sum(axis=1)
            YY = (wr * r).sum() - Y * Y
            YC, YS = (wr * c).sum(axis=1) - Y * C, (wr * s).sum(axis=1) - Y * S
            CC, SS = (w * c * c).sum(axis=1) - C * C, (w * s * s).sum(axis=1) - S * S
            CS = (w * c * s).sum(axis=1) - C * S
            D = CC * SS - CS * CS
            den = YY * D
            p = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / den
            power[b] = np.where(den > 0, p, np.nan)
    return power


def peaks_definition(power):
    """(peak_index int32 [..., n], peak_power [..., n]) of power [..., n, F]: numpy's argmax and max over the frequencies (a NaN
    power counts as the largest), -1 and NaN for a row that is NaN throughout (an invalid orbit)."""
    power = np.asarray(power, dtype=np.float64)
    idx = np.argmax(power, axis=-1).astype(np.int32)
    pk = np.take_along_axis(power, idx[..., None].astype(np.int64), axis=-1)[..., 0]
    dead = np.all(np.isnan(power), axis=-1)
    return np.where(dead, np.int32(-1), idx).astype(np.int32), np.where(dead, np.nan, pk)


def residual_gls(results, model, f0=None, df=None, nfreq=None, keep_planet=None, ndraws=256, nsamples=200,
                 quantiles=predictive.QUANTILES, seed=0, mode="random", bootstrap=True, device=0, return_replicates=False):
    """The posterior band of the residual periodogram from finished runs (a list of NestedResult with samples and logl_birth) of
    `model` (a GpuRVModel).  Every replicate of the merged run (merge.py: mode / bootstrap / seed) gives ndraws equal-weight
    draws (draws.samples); the residuals of every draw (residuals_definition; keep_planet=p leaves planet p's signal in) give a
    periodogram on the grid f0 + df k, k < nfreq (default: frequency_grid(model.table.time)); per frequency the draws' powers
    give the quantiles `quantiles` and the mean (predictive.bands_definition), and the replicates that have draws give the
    statistics of those.  A dict: band [Q, F] (the mean over the replicates), band_err (their standard deviation, ddof 0),
    band_min, band_max, mean, mean_err [F], n_valid_min [F], replicates, freq, period [F], quantiles, and peak_fraction,
    peak_fraction_err [F]: the share of a replicate's draws whose highest peak is at each frequency, as mean and standard
    deviation over the replicates.  With return_replicates also q [S, Q, F], mean_replicates [S, F], peak_index [S, n] and
    alive [S].

    device=k draws and reduces on device k (model.gls_bands); device=None runs the numpy definitions on what
    model.residuals_batch returns."""
    levels = predictive.check_levels(quantiles)
    if f0 is None or df is None or nfreq is None:
        g0, gd, gn = frequency_grid(model.table.time)
        f0, df, nfreq = (g0 if f0 is None else f0), (gd if df is None else df), (gn if nfreq is None else nfreq)
    f0, df, nfreq = check_grid(f0, df, nfreq, np.asarray(model.table.time).shape[0])
    theta = draws.samples(results, ndraws, nsamples, seed, mode, bootstrap, device)          # [S, n, ndim]
    alive = ~np.isnan(theta[:, 0, 0])
    if not alive.any():
        raise ValueError("no replicate of the merged run has weight: nothing to draw from")
    # a replicate without draws is left out below; until then it stands in with the first live replicate's rows
    theta = np.where(alive[:, None, None], theta, theta[int(np.argmax(alive))][None])
    S, n = theta.shape[:2]
    if device is None:
        res, var = model.residuals_batch(theta.reshape(-1, theta.shape[2]), keep_planet=keep_planet)
        power = gls_definition(model.table.time, res, var, f0, df, nfreq).reshape(S, n, nfreq)
        q, mean, nv = predictive.bands_definition(power, levels)
        pidx, _ = peaks_definition(power)
    else:
        got = model.gls_bands(theta, f0, df, nfreq, levels, keep_planet=keep_planet)
        q, mean, nv, pidx = got["q"], got["mean"], got["n_valid"], got["peak_index"]
    frac = np.zeros((S, nfreq))
    for s in range(S):
        hit = pidx[s][pidx[s] >= 0]
        if hit.shape[0]:
            frac[s] = np.bincount(hit, minlength=nfreq) / hit.shape[0]
    band, band_err, band_min, band_max = predictive._over_replicates(q, alive)
    mean_, mean_err, _, _ = predictive._over_replicates(mean, alive)
    pf, pf_err, _, _ = predictive._over_replicates(frac, alive)
    freq = f0 + df * np.arange(nfreq, dtype=np.float64)
    out = dict(band=band, band_err=band_err, band_min=band_min, band_max=band_max, mean=mean_, mean_err=mean_err,
               n_valid_min=nv[alive].min(axis=0), replicates=int(alive.sum()), freq=freq, period=1.0 / freq, quantiles=levels,
               peak_fraction=pf, peak_fraction_err=pf_err)
    if return_replicates:
        out.update(q=q, mean_replicates=mean, peak_index=pidx, alive=alive)
    return out
