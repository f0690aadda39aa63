"""Posterior summaries of merged nested-sampling runs with run-to-run error bars (Higson et al. 2018, "Sampling errors in nested
sampling parameter estimation"): for every replicate of the merged run (merge.py: simulated shrinkage, optionally on top of a
bootstrap of the runs) and every column of `values` — a parameter or a quantity derived from the parameters — the weighted mean,
the weighted standard deviation and weighted quantiles.  The standard deviation of each over the replicates is its error bar.
The numpy definition below is the reference that the device entry (rvll_posterior_replicates;
csrc/rvll_posterior.hip) reproduces; on the device the replicated weights are reduced where they are written and never cross to
the host.

Replicate s has exactly the weights of merge.replicates_arrays(..., return_logwt=True)[2][s]: the same seeds, the same bootstrap
multiplicities, the same merged order.  With p_i = exp(logwt_i) (0 for a row without weight), P = sum p and x_i the column's value
in merged row i:

    mean        sum p_i x_i / P
    std         sqrt(sum p_i (x_i - mean)^2 / P): the spread about the replicate's own mean, not E[x^2] - mean^2
    quantile    the inverted weighted CDF: with the rows sorted by x and c_j the inclusive running sum of p in that order over
                its last entry (summed in np.longdouble, rounded once per row), x of the first j with c_j >= q.  This is
                np.quantile(x, q, weights=p, method="inverted_cdf"); it does not depend on the order of tied x.
    logz, information   as merge.replicates_arrays gives them

A replicate in which no row has weight (a bootstrap that drew only empty runs) has no posterior: its summaries are NaN.

`table` is what the reference's post_processing.py prints after a run — mean, standard deviation, median and the 15.865 / 84.135 %
quantiles of every parameter, the maximum-likelihood row — computed from the merged run's expected weights, with the replicates'
scatter as the error of each; `order_planets` is its period ordering of the planets, vectorised.
"""
import ctypes as C

import numpy as np

from . import _abi, merge
from .shrinkage import replicate_seeds

QUANTILES = (0.15865, 0.5, 0.84135)      # post_processing.py's percentiles 15.865, 50, 84.135
MAX_COLUMNS = 64
MAX_QUANTILES = 16
_BLOCK_ELEMS = 1 << 21                   # (replicate, row) elements the numpy definition holds at a time, per array
_M64 = 2 ** 64 - 1


def table_bytes(nrows, ncols):
    """Bytes of the device's per-call tables: the values in merged order (8 a value) and one permutation a column (4 a row).
    block_bytes must hold them and at least one replicate of the weights, 8 * nrows bytes."""
    return 12 * int(nrows) * int(ncols)


def check_args(values, logl, quantiles):
    """values as float64 [N, C] (C-contiguous) and quantiles as float64 [Q]; raises ValueError where rvll_posterior_replicates
    returns RVLL_E_INVALID for them."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim == 1:
        values = values[:, None]
    if values.ndim != 2:
        raise ValueError("values must be [rows, columns]")
    values = np.ascontiguousarray(values)
    if values.shape[0] != np.asarray(logl).reshape(-1).shape[0]:
        raise ValueError(f"values has {values.shape[0]} rows, logl {np.asarray(logl).reshape(-1).shape[0]}")
    if not 1 <= values.shape[1] <= MAX_COLUMNS:
        raise ValueError(f"need 1 to {MAX_COLUMNS} columns, got {values.shape[1]}")
    if not np.isfinite(values).all():
        raise ValueError("values must be finite: no NaN, no infinity")
    quantiles = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
    if not 1 <= quantiles.shape[0] <= MAX_QUANTILES:
        raise ValueError(f"need 1 to {MAX_QUANTILES} quantile levels, got {quantiles.shape[0]}")
    if not np.all((quantiles > 0.0) & (quantiles < 1.0)):
        raise ValueError("quantile levels must lie in the open interval (0, 1)")
    return values, quantiles


def _reduce(p, xt, perms, xsorted, quantiles, mean, std, quant):
    """One replicate: the weights p [N] in merged order, the columns xt [C, N] in merged order, perms / xsorted [C, N] the rows
    of every column by value.  Fills mean [C], std [C], quant [Q, C]."""
    total = p.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(xt.shape[0]):
            mean[c] = (p * xt[c]).sum() / total
            d = xt[c] - mean[c]
            std[c] = np.sqrt((p * d * d).sum() / total)
            if not total > 0.0:
                quant[:, c] = np.nan
                continue
            cs = np.cumsum(p[perms[c]].astype(np.longdouble))
            cdf = (cs / cs[-1]).astype(np.float64)
            quant[:, c] = xsorted[c][np.searchsorted(cdf, quantiles, side="left")]


def _definition(values, logl, birth, run_start, quantiles, nsamples, code, bootstrap, seed):
    lay = merge._layout(logl, birth, run_start)
    N, R, ncols, nq = logl.shape[0], lay["R"], values.shape[1], quantiles.shape[0]
    xt = np.ascontiguousarray(values[lay["order"]].T)
    perms = np.stack([np.argsort(col, kind="stable") for col in xt])
    xsorted = np.take_along_axis(xt, perms, axis=1)
    seeds = replicate_seeds(seed, nsamples)
    logz, info = np.empty(nsamples), np.empty(nsamples)
    mean, std, quant = np.empty((nsamples, ncols)), np.empty((nsamples, ncols)), np.empty((nsamples, nq, ncols))
    step = max(1, _BLOCK_ELEMS // N)
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        w = merge.bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, _ = merge._block(lay, w, seeds[s0:s1], code == _abi.SHRINK_EXPECTED)
        for s in range(s0, s1):
            with np.errstate(invalid="ignore"):
                p = np.exp(logw[s - s0] - logz[s])
            _reduce(p, xt, perms, xsorted, quantiles, mean[s], std[s], quant[s])
    return logz, info, mean, std, quant


def _device(values, logl, birth, run_start, quantiles, nsamples, code, bootstrap, seed, device, block_bytes, timing):
    lib = _abi.load()
    N, R, ncols, nq = logl.shape[0], run_start.shape[0] - 1, values.shape[1], quantiles.shape[0]
    logz, info = np.empty(nsamples), np.empty(nsamples)
    mean, std, quant = np.empty((nsamples, ncols)), np.empty((nsamples, ncols)), np.empty((nsamples, nq, ncols))
    t = _abi.PosteriorTiming()
    _abi.check(lib.rvll_posterior_replicates(
        int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(C.POINTER(C.c_int64)), R,
        _abi.as_dp(values), ncols, _abi.as_dp(quantiles), nq, nsamples, code, 1 if bootstrap else 0, int(seed) & _M64,
        _abi.as_dp(logz), _abi.as_dp(info), _abi.as_dp(mean), _abi.as_dp(std), _abi.as_dp(quant), int(block_bytes or 0),
        C.byref(t)))
    if timing is not None:
        timing.update({name: getattr(t, name) for name, _ in t._fields_ if name != "reserved"})
    return logz, info, mean, std, quant


def summarize_arrays(values, logl, birth, run_start, quantiles=QUANTILES, nsamples=1000, seed=0, mode="random", bootstrap=True,
                     device=None, block_bytes=None, timing=None):
    """Summaries of `values` (float64 [N, C] in input row order, finite, 1 <= C <= 64) over nsamples replicates of the merged
    run of the runs (logl, birth, run_start) as merge.replicates_arrays takes them: a dict with mean [S, C], std [S, C],
    quantiles [S, Q, C] (the levels `quantiles`, each in (0, 1), Q <= 16), logz [S] and information [S].  device=None evaluates
    the numpy definition, in blocks of replicates; device=k runs rvll_posterior_replicates on device k (block_bytes bounds the
    device tables, table_bytes(N, C), plus the block of weights; default: the tables plus 8 GiB, of which no more than nsamples
    replicates are allocated; timing: a dict that receives the call's rvll_posterior_timing)."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    values, quantiles = check_args(values, logl, quantiles)
    fn = _definition if device is None else _device
    extra = () if device is None else (device, block_bytes, timing)
    logz, info, mean, std, quant = fn(values, logl, birth, run_start, quantiles, nsamples, code, bootstrap, seed, *extra)
    return dict(mean=mean, std=std, quantiles=quant, logz=logz, information=info)


def _planet_blocks(parnames):
    """The column indexes of planet1_*, planet2_*, ... (one list a planet, in the order of parnames) and the position of the
    period inside a block."""
    parnames = list(parnames)
    blocks = []
    while True:
        prefix = f"planet{len(blocks) + 1}_"
        cols = [i for i, name in enumerate(parnames) if name.startswith(prefix)]
        if not cols:
            break
        blocks.append(cols)
    if not blocks:
        return blocks, None
    if len({len(b) for b in blocks}) != 1:
        raise ValueError("every planet needs the same number of columns to be matched by position")
    pos = []
    for n, b in enumerate(blocks):
        where = [k for k, i in enumerate(b) if "period" in parnames[i]]
        if not where:
            raise ValueError(f"planet{n + 1} has no period column")
        pos.append(where[0])
    if len(set(pos)) != 1:
        raise ValueError("the period must sit at the same position in every planet's block")
    return blocks, pos[0]


def order_planets(samples, parnames):
    """A new array in which, row by row, the blocks of planet{n}_* columns are permuted so that planet1_period <=
    planet2_period <= ... (ties keep their order; rows already ordered come back unchanged; columns of no planet stay).  The
    columns of two planets are matched by their position within the planet's block, as the reference's post_processing.py
    does, so planet 1 may carry ecc / omega where planet 2 carries secos / sesin.  Periods are compared as stored.  One
    vectorised pass instead of the reference's per-row loop."""
    out = np.array(samples, dtype=np.float64, copy=True)
    if out.ndim != 2 or out.shape[1] != len(parnames):
        raise ValueError("samples must be [rows, len(parnames)]")
    blocks, pos = _planet_blocks(parnames)
    if len(blocks) < 2:
        return out
    blk = np.asarray(blocks)                                  # [P, B]
    data = out[:, blk]                                        # [N, P, B]
    rank = np.argsort(data[:, :, pos], axis=1, kind="stable")
    out[:, blk] = np.take_along_axis(data, rank[:, :, None], axis=1)
    return out


def _values(results, columns, derived, order, parnames):
    results, logl, birth, run_start = merge._stack(results)
    for i, res in enumerate(results):
        if getattr(res, "samples", None) is None or len(res.samples) != len(res.logl):
            raise ValueError(f"result {i} has no samples for its rows")
    samples = np.concatenate([np.asarray(res.samples, dtype=np.float64).reshape(len(res.logl), -1) for res in results])
    if order:
        if parnames is None:
            raise ValueError("order=True needs parnames")
        samples = order_planets(samples, parnames)
    if columns is None:
        cols = samples
    else:
        idx = [list(parnames).index(c) if isinstance(c, str) else int(c) for c in columns]
        cols = samples[:, idx]
    if derived is not None:
        extra = np.asarray(derived(samples), dtype=np.float64)
        extra = extra[:, None] if extra.ndim == 1 else extra
        if extra.ndim != 2 or extra.shape[0] != samples.shape[0]:
            raise ValueError("derived must return [rows, extra columns]")
        cols = np.concatenate([cols, extra], axis=1)
    return samples, np.ascontiguousarray(cols), logl, birth, run_start


def summarize(results, columns=None, derived=None, order=False, parnames=None, **kw):
    """summarize_arrays for finished runs (a list of NestedResult with samples and logl_birth, stacked as merge.merge stacks
    them).  columns: the sample columns to summarise (indexes, or names looked up in parnames; default all); derived: a
    callable from samples [N, D] to extra columns [N, E], appended after them (the eccentricity from secos / sesin, say);
    order=True applies order_planets(samples, parnames) first.  The other keywords are summarize_arrays'."""
    _, cols, logl, birth, run_start = _values(results, columns, derived, order, parnames)
    return summarize_arrays(cols, logl, birth, run_start, **kw)


def table(results, parnames, columns=None, derived=None, derived_names=(), order=False, nsamples=1000, seed=0, mode="random",
          bootstrap=True, device=None, block_bytes=None, timing=None):
    """The table the reference's post-processing prints, with error bars.  Per summarised column (names: the chosen parnames,
    then derived_names): mean, std, median, lower and upper (the 15.865 / 84.135 % quantiles) from the merged run's expected
    weights (mode="expected", no bootstrap, one replicate), and mean_err, std_err, median_err, lower_err, upper_err, the
    standard deviation of each over nsamples replicates (mode / bootstrap / seed; bootstrap=False leaves the shrinkage error
    alone).  Also max_loglike and max_loglike_row (the last merged row's log-L and samples, after the ordering if order=True),
    logz (expected) and logz_err.  A dict of plain arrays; format_table turns it into text."""
    samples, cols, logl, birth, run_start = _values(results, columns, derived, order, parnames)
    names = list(parnames) if columns is None else [c if isinstance(c, str) else list(parnames)[int(c)] for c in columns]
    names += list(derived_names)
    if len(names) != cols.shape[1]:
        raise ValueError(f"{cols.shape[1]} columns but {len(names)} names (derived_names must name every derived column)")
    point = summarize_arrays(cols, logl, birth, run_start, QUANTILES, 1, seed, "expected", False, device, block_bytes)
    reps = summarize_arrays(cols, logl, birth, run_start, QUANTILES, nsamples, seed, mode, bootstrap, device, block_bytes, timing)
    top = logl.shape[0] - 1 - int(np.argmax(logl[::-1]))      # the last merged row: the highest log-L, the last of its ties
    out = dict(names=names, nsamples=int(nsamples), mean=point["mean"][0], std=point["std"][0], lower=point["quantiles"][0, 0],
               median=point["quantiles"][0, 1], upper=point["quantiles"][0, 2], mean_err=np.std(reps["mean"], axis=0),
               std_err=np.std(reps["std"], axis=0), lower_err=np.std(reps["quantiles"][:, 0], axis=0),
               median_err=np.std(reps["quantiles"][:, 1], axis=0), upper_err=np.std(reps["quantiles"][:, 2], axis=0),
               max_loglike=float(logl[top]), max_loglike_row=samples[top].copy(), logz=float(point["logz"][0]),
               logz_err=float(np.std(reps["logz"])), replicates=reps)
    return out


def format_table(tab, other=None, labels=("+/-", "+/-")):
    """Text of a table(...) dict, one line a column: value and error of mean, std, median, lower and upper.  other: a second
    table of the same columns (the shrinkage-only one, say) whose errors are printed next to the first's."""
    keys = ("mean", "std", "median", "lower", "upper")
    width = max(len(n) for n in tab["names"])
    head = f"{'':{width}s}" + "".join(f"  {k:>13s} {labels[0]:>9s}" + (f" {labels[1]:>9s}" if other else "") for k in keys)
    lines = [head]
    for c, name in enumerate(tab["names"]):
        line = f"{name:{width}s}"
        for k in keys:
            line += f"  {tab[k][c]:13.7g} {tab[k + '_err'][c]:9.2e}"
            if other:
                line += f" {other[k + '_err'][c]:9.2e}"
        lines.append(line)
    lines.append(f"ln Z = {tab['logz']:.4f} +/- {tab['logz_err']:.4f}   max log-L = {tab['max_loglike']:.4f}   "
                 f"({tab['nsamples']} replicates)")
    return "\n".join(lines)
