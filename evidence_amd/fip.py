"""FIP periodogram (Hara et al. 2021) accumulation on the GPU — the data-parallel part of
evidence/fip_criterion.py.

The reference script walks a directory of finished runs, unpickles their posteriors and then runs, per
independent run, a Python loop over every posterior sample of every planet model that subtracts
p(k|y)·w_i from every frequency bin within half a window of one of the sample's orbital frequencies
(fip_criterion.py:305-339).  Here the loop is `rvll_fip_accumulate` (include/rvll.h): the host only flattens
the posteriors into rows in the reference's loop order; the result is bit-identical.

`merged_tip_arrays` and `merged_fip` are the periodogram of the runs of every model merged by their birth
contours (merge.py), with the scatter over simulated-shrinkage and run-bootstrap replicates as the error bar of log10 FIP at every
frequency and of p(k | y).  Their numpy definition is below; the device entry is `rvll_fip_replicates`
(csrc/rvll_fip_merged.hip), which reduces the replicated weights where they are written.

Not reproduced: the directory walk / pickle loading (:50-220, sampler-output specific), the `--with-alias`
branch (:322-332 reads `x_freqs` before assigning it — it raises NameError upstream) and the plots.
"""
import ctypes as C

import numpy as np
from scipy.special import logsumexp

from . import _abi, merge
from .shrinkage import SEED_MUL, replicate_seeds

NFREQ = 50000                 # fip_criterion.py:229
COEF_WINDOW = 1.0             # :230


def frequency_grid(pmin, pmax, tobs, nfreq=NFREQ, coef_window=COEF_WINDOW):
    """nu, nua, nub of fip_criterion.py:233-236 (angular frequencies, rad/day)."""
    nu = np.linspace(2 * np.pi / pmax, 2 * np.pi / pmin, nfreq)
    nu_window = coef_window * 2 * np.pi / tobs
    return nu, nu - nu_window / 2, nu + nu_window / 2


def observation_span(datadict):
    """Tobs of :206-222: max - min over all instruments of the `rjd` (else `jdb`) column."""
    lo, hi = 1e9, 0.0
    for inst in datadict.values():
        data = inst["data"]
        t = data["rjd"].values if "rjd" in data else data["jdb"].values
        lo, hi = min(lo, float(np.min(t))), max(hi, float(np.max(t)))
    return hi - lo


def model_probabilities(logzs_per_run):
    """p(k | y) from the per-model median of ln Z over the runs (:243-270).  logzs_per_run[r][k]."""
    logzs = np.median(np.asarray(logzs_per_run, dtype=float), axis=0)
    return np.exp(logzs - logsumexp(logzs))


def flatten_posteriors(posteriors, pky):
    """posteriors[r][k] = (samples [n, k], weights [n]) for k >= 1 (entry 0 — the no-planet model — is
    ignored, it has no periods) -> periods [rows, np_max] NaN-padded, contrib [rows], run_start [R + 1],
    in the reference's loop order: run, then kmod, then sample (:310-319)."""
    np_max = max((np.atleast_2d(p[0]).shape[1] for per_k in posteriors for p in per_k[1:] if p is not None),
                 default=1)
    if np_max > _abi.FIP_MAX_PLANETS:
        raise ValueError(f"more than {_abi.FIP_MAX_PLANETS} periods per sample")
    entries, run_start, rows = [], [0], 0
    for per_k in posteriors:
        for kmod in range(1, len(per_k)):
            if per_k[kmod] is None:
                continue
            samples, weights = per_k[kmod]
            samples = np.asarray(samples, dtype=np.float64)
            samples = samples.reshape(len(samples), -1)
            if len(weights) != len(samples):
                raise ValueError("one weight per sample required")
            entries.append((rows, kmod, samples, weights))
            rows += len(samples)
        run_start.append(rows)
    periods = np.empty((rows, np_max))
    contrib = np.empty(rows)
    for lo, kmod, samples, weights in entries:
        hi, k = lo + len(samples), samples.shape[1]
        periods[lo:hi, :k] = samples
        periods[lo:hi, k:] = np.nan
        np.divide(weights, np.sum(weights), out=contrib[lo:hi])              # :315  weights /= np.sum(weights)
        np.multiply(pky[kmod], contrib[lo:hi], out=contrib[lo:hi])            # :339  pky[kmod]*weights[i]
    return periods, contrib, np.asarray(run_start, dtype=np.int64)


def fip_periodogram(posteriors, pky, nua, nub, device=-1, repeats=1, return_timing=False):
    """fapnu [R, nfreq]: 1 - sum over models and samples of p(k|y) w_i [bin within the window of a sample
    frequency], accumulated on the GPU in the reference's order (bit-identical to :305-339)."""
    lib = _abi.load()
    nua = np.ascontiguousarray(nua, dtype=np.float64)
    nub = np.ascontiguousarray(nub, dtype=np.float64)
    if nua.shape != nub.shape or nua.ndim != 1:
        raise ValueError("nua and nub must be 1-D arrays of one length")
    periods, contrib, run_start = flatten_posteriors(posteriors, np.asarray(pky, dtype=np.float64))
    fapnu = np.ones((len(posteriors), nua.size))                              # :307
    timing = _abi.FipTiming()
    _abi.check(lib.rvll_fip_accumulate(
        int(device), _abi.as_dp(nua), _abi.as_dp(nub), nua.size, _abi.as_dp(periods), _abi.as_dp(contrib),
        run_start.ctypes.data_as(C.POINTER(C.c_int64)), len(posteriors), periods.shape[1], _abi.as_dp(fapnu),
        int(repeats), C.byref(timing)))
    if return_timing:
        return fapnu, {"index_ms": timing.index_ms, "accumulate_ms": timing.accumulate_ms, "rows": timing.rows,
                       "repeats": timing.repeats}
    return fapnu


def fip_summary(fapnu, nu):
    """The statistics the script derives from the matrix (:347-388): clipped log10 FIP per run, the
    convergence test (max - min over runs > 1 dex), median / std over runs and the mean FIP."""
    cut = np.maximum(fapnu, 1e-15)
    log10fips = np.log10(cut)
    diffs = np.max(log10fips, axis=0) - np.min(log10fips, axis=0)
    failed = np.where(diffs > 1)[0]
    return {"log10fips": log10fips, "diffs": diffs, "converged": failed.size == 0,
            "failed_periods": 2 * np.pi / np.asarray(nu)[failed],
            "median": np.median(log10fips, axis=0), "std": np.std(log10fips, axis=0),
            "mean": np.mean(cut, axis=0), "periods": 2 * np.pi / np.asarray(nu)}


# ---- the periodogram of merged runs ---------------------------------------------------------------------
# seed_k = seed + k * MODEL_SEED_MUL mod 2^64 is the seed of planet model k in merged_fip.  An odd 64-bit constant (the first
# multiplier of wyhash), unrelated to SEED_MUL (the step from replicate to replicate) and to 0x9E3779B97F4A7C15 (the step from
# counter to counter inside uniform01): with either of those, model k's draws would be model 0's shifted by k.
MODEL_SEED_MUL = 0xA0761D6478BD642F
FIP_FLOOR = 1e-15                        # fip_criterion.py:354 clips the FIP here before the log10
_BLOCK_ELEMS = 1 << 21                   # (replicate, event) elements the numpy definition holds at a time, per array
_HOST_BLOCK_ELEMS = 1 << 24              # (replicate, bin) elements of one model that merged_fip holds at a time
_M64 = 2 ** 64 - 1
_TWO_PI = 6.283185307179586


def merged_table_bytes(nrows, nplanets, nfreq):
    """Bytes of the device's per-call tables in rvll_fip_replicates: two event lists of 4-byte positions, two count tables over
    the bins and two tile tables.  block_bytes must hold them and at least one replicate, 8 * nrows + 16 * nfreq bytes."""
    m = int(nrows) * int(nplanets)
    return 8 * m + 8 * int(nfreq) + 8 * ((m + 1023) // 1024 + 1)


def check_merged_args(periods, logl, nua, nub):
    """periods as float64 [N, np] (C-contiguous), nua and nub as float64 [nfreq]; raises ValueError where rvll_fip_replicates
    returns RVLL_E_INVALID for them."""
    periods = np.asarray(periods, dtype=np.float64)
    if periods.ndim == 1:
        periods = periods[:, None]
    if periods.ndim != 2:
        raise ValueError("periods must be [rows, planets]")
    periods = np.ascontiguousarray(periods)
    nrows = np.asarray(logl).reshape(-1).shape[0]
    if periods.shape[0] != nrows:
        raise ValueError(f"periods has {periods.shape[0]} rows, logl {nrows}")
    if not 1 <= periods.shape[1] <= _abi.FIP_MAX_PLANETS:
        raise ValueError(f"need 1 to {_abi.FIP_MAX_PLANETS} periods a row, got {periods.shape[1]}")
    if periods.size > 2 ** 31 - 1:
        raise ValueError("rows * planets must stay below 2^31")
    if not (np.isfinite(periods).all() and (periods > 0.0).all()):
        raise ValueError("periods must be finite and positive")
    nua = np.ascontiguousarray(nua, dtype=np.float64)
    nub = np.ascontiguousarray(nub, dtype=np.float64)
    if nua.ndim != 1 or nua.shape != nub.shape or not 1 <= nua.size <= 2 ** 30:
        raise ValueError("nua and nub must be 1-D arrays of one length, 1 to 2^30 bins")
    if np.isnan(nua).any() or np.isnan(nub).any() or np.any(np.diff(nua) < 0) or np.any(np.diff(nub) < 0):
        raise ValueError("nua and nub must be non-decreasing, without NaN")
    return periods, nua, nub


def row_intervals(periods, nua, nub):
    """(beg, end) int64 [N, np]: per row the union of its spans (fip_criterion.py:333-334) as disjoint, non-touching intervals
    in rising order; the unused slots of a row hold (nfreq, nfreq)."""
    nfreq = nua.shape[0]
    omega = _TWO_PI / periods
    beg = np.searchsorted(nub, omega, "right").astype(np.int64)
    end = np.searchsorted(nua, omega, "left").astype(np.int64)
    big = np.iinfo(np.int64).max
    empty = beg >= end
    beg[empty] = end[empty] = big
    by = np.argsort(beg, axis=1, kind="stable")
    beg, end = np.take_along_axis(beg, by, axis=1), np.take_along_axis(end, by, axis=1)
    nrows, nplanets = beg.shape
    out_b, out_e = np.full((nrows, nplanets), nfreq, np.int64), np.full((nrows, nplanets), nfreq, np.int64)
    cnt = np.zeros(nrows, np.int64)
    cb, ce = beg[:, 0].copy(), end[:, 0].copy()
    for j in range(1, nplanets):
        valid = beg[:, j] != big
        join = valid & (beg[:, j] <= ce)                     # overlapping or adjacent
        ce[join] = np.maximum(ce[join], end[join, j])
        new = np.flatnonzero(valid & ~join)
        out_b[new, cnt[new]], out_e[new, cnt[new]] = cb[new], ce[new]
        cnt[new] += 1
        cb[new], ce[new] = beg[new, j], end[new, j]
    last = np.flatnonzero(cb != big)
    out_b[last, cnt[last]], out_e[last, cnt[last]] = cb[last], ce[last]
    return out_b, out_e


def _event_list(keys, nfreq):
    """One event list: the merged positions of the events with bin < nfreq in (bin, merged position) order, and per bin b the
    number of events with bin <= b."""
    nplanets = keys.shape[1]
    flat = keys.reshape(-1)
    by = np.argsort(flat, kind="stable")
    cnt = np.searchsorted(flat[by], np.arange(nfreq), "right")
    return (by[:cnt[-1]] // nplanets).astype(np.int64), cnt


def _prepare(periods, logl, birth, run_start, nua, nub):
    lay = merge._layout(logl, birth, run_start)
    beg, end = row_intervals(periods[lay["order"]], nua, nub)
    pos_a, cnt_a = _event_list(beg, nua.shape[0])
    pos_e, cnt_e = _event_list(end, nua.shape[0])
    return dict(lay=lay, pos_a=pos_a, cnt_a=cnt_a, pos_e=pos_e, cnt_e=cnt_e, nfreq=nua.shape[0],
                step=max(1, _BLOCK_ELEMS // max(1, periods.size)))


def _running(p, pos, cnt):
    """[S_b, nfreq]: per replicate the running sum of p[pos] in np.longdouble, rounded once, read after cnt[b] events."""
    cs = np.cumsum(p[:, pos].astype(np.longdouble), axis=1).astype(np.float64)
    return np.concatenate([np.zeros((p.shape[0], 1)), cs], axis=1)[:, cnt]


def _definition_block(prep, seeds, expected, bootstrap, parts=False):
    """The replicates with the seeds `seeds` of a prepared model: (logz, information, tip [len(seeds), nfreq])."""
    lay, R, S = prep["lay"], prep["lay"]["R"], seeds.shape[0]
    logz, info, tip = np.empty(S), np.empty(S), np.empty((S, prep["nfreq"]))
    a_all, e_all = (np.empty_like(tip), np.empty_like(tip)) if parts else (None, None)
    covered = prep["cnt_a"] != prep["cnt_e"]
    for s0 in range(0, S, prep["step"]):
        s1 = min(S, s0 + prep["step"])
        w = merge.bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, _ = merge._block(lay, w, seeds[s0:s1], expected)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.exp(logw - logz[s0:s1, None])
            total = p.sum(axis=1)
            a, e = _running(p, prep["pos_a"], prep["cnt_a"]), _running(p, prep["pos_e"], prep["cnt_e"])
            t = np.where(covered[None, :], np.clip((a - e) / total[:, None], 0.0, 1.0), 0.0)
            t[~(total > 0.0)] = np.nan
        tip[s0:s1] = t
        if parts:
            a_all[s0:s1], e_all[s0:s1] = a / total[:, None], e / total[:, None]
    return (logz, info, tip, a_all, e_all) if parts else (logz, info, tip)


def _device_tip(periods, logl, birth, run_start, nua, nub, nsamples, code, bootstrap, seed, device, block_bytes, timing):
    lib = _abi.load()
    N, R, nfreq = logl.shape[0], run_start.shape[0] - 1, nua.shape[0]
    logz, info, tip = np.empty(nsamples), np.empty(nsamples), np.empty((nsamples, nfreq))
    t = _abi.FipMergedTiming()
    _abi.check(lib.rvll_fip_replicates(
        int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(C.POINTER(C.c_int64)), R,
        _abi.as_dp(periods), periods.shape[1], _abi.as_dp(nua), _abi.as_dp(nub), nfreq, nsamples, code, 1 if bootstrap else 0,
        int(seed) & _M64, _abi.as_dp(logz), _abi.as_dp(info), _abi.as_dp(tip), int(block_bytes or 0), C.byref(t)))
    if timing is not None:
        timing.update({name: getattr(t, name) for name, _ in t._fields_})
    return logz, info, tip


def merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=1000, seed=0, mode="random", bootstrap=True,
                      device=None, block_bytes=None, timing=None):
    """The true inclusion probability of every frequency bin over nsamples replicates of the merged run of the runs (logl,
    birth, run_start) as merge.replicates_arrays takes them: a dict with tip [S, nfreq], logz [S] and information [S].
    periods is float64 [N, np] in input row order, finite and positive, 1 <= np <= 8; nua and nub are non-decreasing [nfreq]
    (frequency_grid).  Replicate s has the weights of merge.replicates_arrays(..., return_logwt=True)[2][s]: p = exp(logwt), 0
    for a row without weight, P = sum p.  Row i covers the union of the spans [#{nub <= w}, #{nua < w}), w = 2 pi / P_ij, of its
    periods (a bin once, as the reference's fancy-index -= does), and

        tip[s, b] = sum of p over the rows that cover b, over P
                  = (A[b] - E[b]) / P,  A[b] (E[b]) = sum of p over the row intervals with beg <= b (end <= b)

    with the rows' covers written as disjoint, non-touching intervals (row_intervals).  A and E are running sums over the events
    in (bin, merged position) order, taken in np.longdouble and rounded once per bin.  A bin that no interval covers is exactly 0,
    decided from the integer counts of open intervals; tip is clamped to [0, 1]; a replicate in which no row has weight is NaN.
    device=None evaluates this definition in blocks of replicates; device=k runs rvll_fip_replicates on device k (block_bytes
    bounds merged_table_bytes(N, np, nfreq) plus 8 N + 16 nfreq bytes a replicate of the block; default: the tables plus 8 GiB,
    of which no more than nsamples replicates are allocated; timing: a dict that receives the call's rvll_fip_merged_timing)."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    periods, nua, nub = check_merged_args(periods, logl, nua, nub)
    if device is None:
        prep = _prepare(periods, logl, birth, run_start, nua, nub)
        logz, info, tip = _definition_block(prep, replicate_seeds(seed, nsamples), code == _abi.SHRINK_EXPECTED, bootstrap)
    else:
        logz, info, tip = _device_tip(periods, logl, birth, run_start, nua, nub, nsamples, code, bootstrap, seed, device,
                                      block_bytes, timing)
    return dict(tip=tip, logz=logz, information=info)


def model_seed(seed, k):
    """The seed of planet model k in merged_fip: (seed + k * MODEL_SEED_MUL) mod 2^64."""
    return (int(seed) + int(k) * MODEL_SEED_MUL) & _M64


class _Moments:
    """Count, mean and sum of squared deviations of the rows seen so far, per column (Chan et al.'s pairwise update), and
    their minimum and maximum: the statistics of all replicates from one block at a time."""

    def __init__(self):
        self.n, self.mean, self.m2, self.min, self.max = 0, None, None, None, None

    def add(self, x):
        nb, mb = x.shape[0], x.mean(axis=0)
        m2b = ((x - mb) ** 2).sum(axis=0)
        if self.n == 0:
            self.n, self.mean, self.m2, self.min, self.max = nb, mb, m2b, x.min(axis=0), x.max(axis=0)
            return
        d, n = mb - self.mean, self.n + nb
        self.m2 = self.m2 + m2b + d * d * (self.n * nb / n)
        self.mean = self.mean + d * (nb / n)
        self.min, self.max, self.n = np.minimum(self.min, x.min(axis=0)), np.maximum(self.max, x.max(axis=0)), n

    def std(self):
        return np.sqrt(self.m2 / self.n)


def _softmax(logz):
    with np.errstate(invalid="ignore"):
        return np.exp(logz - logsumexp(logz, axis=-1, keepdims=True))


def merged_fip(results_per_model, period_columns, nua, nub, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None,
               return_replicates=False, nu=None, block_bytes=None, replicate_block=None, timing=None):
    """The FIP periodogram of the merged runs of every planet model, with run-to-run error bars.  results_per_model[k] is the
    list of finished runs (NestedResult with samples and logl_birth) of the model with k planets, k = 0 .. K;
    period_columns[k] the sample columns of its periods (empty for k = 0, which contributes its ln Z alone).  Model k is
    replicated with the seed model_seed(seed, k), so the bootstraps of different models are independent draws, as their runs
    are.  Per replicate s:

        pky_s[k] = exp(lnZ_{k,s} - logsumexp_k lnZ_{k,s})            the replicate's own model probabilities
        FIP_s[b] = 1 - sum_{k >= 1} pky_s[k] * tip_{k,s}[b]           tip: merged_tip_arrays

    A dict: fip, log10fip (point values: mode="expected", no bootstrap, one replicate; log10 of max(FIP, 1e-15)); log10fip_err
    (the standard deviation over the replicates of the clipped log10 FIP_s), log10fip_min, log10fip_max; pky, pky_err; logz,
    logz_err [K + 1]; pky_replicates, logz_replicates [S, K + 1]; nsamples; periods = 2 pi / nu when nu is given; and with
    return_replicates the [S, nfreq] array `replicates` of FIP_s.  Otherwise the host holds one block of replicates per model at
    a time (replicate_block replicates; default 2^24 / nfreq): replicates s0 .. s0 + B - 1 are the call with the seed
    seed + s0 * SEED_MUL, and the statistics are accumulated block by block.  A replicate without weight (NaN) makes the errors
    NaN.  device=None: the numpy definition; device=k: rvll_fip_replicates / rvll_merge_replicates (block_bytes: theirs;
    timing: a dict that receives the summed kernel_ms and total_ms of the replicate calls)."""
    K = len(results_per_model) - 1
    if K < 1 or len(period_columns) != K + 1:
        raise ValueError("need the models k = 0 .. K, K >= 1, and one list of period columns for each")
    if len(period_columns[0]) != 0:
        raise ValueError("the model without planets has no period columns")
    nsamples = int(nsamples)
    models = []
    for k in range(K + 1):
        results, logl, birth, run_start = merge._stack(results_per_model[k])
        if k == 0:
            models.append((None, logl, birth, run_start))
            continue
        for i, res in enumerate(results):
            if getattr(res, "samples", None) is None or len(res.samples) != len(res.logl):
                raise ValueError(f"model {k}, result {i} has no samples for its rows")
        cols = [int(c) for c in period_columns[k]]
        per = np.concatenate([np.asarray(res.samples, dtype=np.float64).reshape(len(res.logl), -1)[:, cols] for res in results])
        logl, birth, run_start, _, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
        per, nua, nub = check_merged_args(per, logl, nua, nub)
        models.append((per, logl, birth, run_start))
    nfreq = nua.shape[0]
    preps = [None] + [_prepare(*models[k], nua, nub) for k in range(1, K + 1)] if device is None else None
    spent = dict(kernel_ms=0.0, total_ms=0.0)

    def block(s0, nb, mode_, bootstrap_):
        """logz [nb, K + 1] and FIP [nb, nfreq] of the replicates s0 .. s0 + nb - 1."""
        logz, tips = np.empty((nb, K + 1)), []
        for k in range(K + 1):
            per, logl, birth, run_start = models[k]
            sk = (model_seed(seed, k) + s0 * SEED_MUL) & _M64
            t = {}
            if k == 0:
                logz[:, 0] = merge.replicates_arrays(logl, birth, run_start, nb, sk, mode_, bootstrap_, device=device,
                                                     block_bytes=None, timing=t)[0]
            elif device is None:
                logz[:, k], _, tip = _definition_block(preps[k], replicate_seeds(sk, nb), mode_ == "expected", bootstrap_)
                tips.append(tip)
            else:
                out = merged_tip_arrays(per, logl, birth, run_start, nua, nub, nb, sk, mode_, bootstrap_, device, block_bytes, t)
                logz[:, k] = out["logz"]
                tips.append(out["tip"])
            for key in spent:
                spent[key] += t.get(key, 0.0)
        pky = _softmax(logz)
        fip = np.ones((nb, nfreq))
        for k in range(1, K + 1):
            fip -= pky[:, k, None] * tips[k - 1]
        return logz, pky, fip

    logz0, pky0, fip0 = block(0, 1, "expected", False)
    step = int(replicate_block) if replicate_block else max(1, _HOST_BLOCK_ELEMS // nfreq)
    step = nsamples if return_replicates else max(1, min(step, nsamples))
    logz_s, pky_s = np.empty((nsamples, K + 1)), np.empty((nsamples, K + 1))
    acc, reps = _Moments(), None
    for s0 in range(0, nsamples, step):
        nb = min(step, nsamples - s0)
        logz_s[s0:s0 + nb], pky_s[s0:s0 + nb], fip = block(s0, nb, mode, bootstrap)
        acc.add(np.log10(np.maximum(fip, FIP_FLOOR)))
        if return_replicates:
            reps = fip
    out = dict(fip=fip0[0], log10fip=np.log10(np.maximum(fip0[0], FIP_FLOOR)), log10fip_err=acc.std(), log10fip_min=acc.min,
               log10fip_max=acc.max, pky=pky0[0], pky_err=np.std(pky_s, axis=0), logz=logz0[0], logz_err=np.std(logz_s, axis=0),
               pky_replicates=pky_s, logz_replicates=logz_s, nsamples=nsamples)
    if nu is not None:
        out["periods"] = 2 * np.pi / np.asarray(nu, dtype=np.float64)
    if return_replicates:
        out["replicates"] = reps
    if timing is not None:
        timing.update(spent)
    return out
