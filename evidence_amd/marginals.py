"""Marginal posterior histograms of merged nested-sampling runs with run-to-run error bars: what the reference's
post_processing.py plots — one histogram a parameter and the corner plot of every pair — as numbers, with the scatter of every
bin over the replicates of the merged run (merge.py: simulated shrinkage, optionally on top of a bootstrap of the runs).  A second
bump in a period marginal is real or one run's accident; the per-bin error bar tells the two apart.  The numpy definition below
 is the reference that the device entry (rvll_marginal_replicates; csrc/rvll_marginal.hip) reproduces; on the device
the replicated weights are reduced where they are written and never cross to the host.

An *axis* is a column of `values` and a strictly increasing array of at least 2 finite edges (len(edges) - 1 bins, at most 4096).
A *panel* is one axis (1-D) or two axes (a, b) (2-D, bins row-major with a the major index, at most 4096 bins).  Panel t owns the
bins panel_start[t] .. panel_start[t + 1] of one flat bin array.

    bin         numpy.histogram's convention for explicit edges: j = searchsorted(edges, x, side="right") - 1, x == edges[-1]
                belongs to the last bin, x < edges[0] or x > edges[-1] is outside; doubles compare as doubles (-0.0 == +0.0).
                A row is outside a 2-D panel if it is outside either axis.
    counts      counts[b] the rows in bin b, outside_count[t] the rows outside panel t: integers, the same in every replicate
    mass        replicate s has exactly the weights of merge.replicates_arrays(..., return_logwt=True)[2][s].  With p_i =
                exp(logwt_i) (0 for a row without weight) the row contributes the integer m_i = rint(p_i 2^62) (int64; p <= 1
                because ln Z is a logsumexp, so M = sum m < 2^63), h[b] = sum of m_i over the rows of bin b in int64, and
                mass_s[b] = float64(h[b]) / float64(M); outside_s[t] likewise.  Integer sums do not depend on the order, so any
                schedule agrees exactly on the same m.  A weight below 2^-63 of the total is dropped: 1.1e-19 of the posterior
                mass a row.  A replicate with M = 0 (a bootstrap that drew only empty runs) is NaN throughout.
    statistics  per bin over the replicates s = 0 .. S - 1 in order, NaN replicates skipped, the sequential Welford update
                n += 1; d = x - mean; mean += d / n; m2 += d (x - mean); sd = sqrt(m2 / n) (ddof 0), and the running min and max

`marginals` turns finished runs into the panels of the reference's plots: edges over the [1e-4, 1 - 1e-4] quantile range of the
expected-weight run, linear or (for periods) logarithmic, the point density from the expected weights and its replicate error.
The reference's bins='auto' is not reproduced.  `credible_levels` gives the density thresholds of a corner plot's contours.
"""
import ctypes as C

import numpy as np

from . import _abi, merge, posterior
from .shrinkage import replicate_seeds

MAX_COLUMNS = 64
MAX_AXES = 128
MAX_PANELS = 256
MAX_AXIS_BINS = 4096
MAX_PANEL_BINS = 4096
SCALE = 2.0 ** 62
RANGE_QUANTILES = (1e-4, 1.0 - 1e-4)
_BLOCK_ELEMS = 1 << 21                   # (replicate, row) elements the numpy definition holds at a time, per array
_M64 = 2 ** 64 - 1
_i64p = C.POINTER(C.c_int64)


def table_bytes(nrows, naxes):
    """Bytes of the device's per-call table: one uint16 bin index per (axis, row)."""
    return 2 * int(nrows) * int(naxes)


def replicate_bytes(nrows, nbins, npanels):
    """Bytes one replicate takes in a device block: its weights (8 a row) and its int64 histograms (8 a bin and 8 a panel for
    the rows outside).  block_bytes must hold table_bytes(...) and at least one replicate."""
    return 8 * (int(nrows) + int(nbins) + int(npanels))


def check_args(values, logl, axes, panels):
    """values as float64 [N, C] (C-contiguous), and the axes and panels in the entry's flat form: edges (float64, all axes in a
    row), axis_col int32 [A], axis_edge_start int64 [A + 1], panel_axes int32 [P, 2] (second entry -1 for a 1-D panel),
    panel_start int64 [P + 1].  Raises ValueError where rvll_marginal_replicates returns RVLL_E_INVALID."""
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
    axes, panels = list(axes), list(panels)
    if not 1 <= len(axes) <= MAX_AXES:
        raise ValueError(f"need 1 to {MAX_AXES} axes, got {len(axes)}")
    if not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError(f"need 1 to {MAX_PANELS} panels, got {len(panels)}")
    cols, edge_list = [], []
    for a, (col, edges) in enumerate(axes):
        edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if not 2 <= edges.shape[0] <= MAX_AXIS_BINS + 1:
            raise ValueError(f"axis {a}: need 2 to {MAX_AXIS_BINS + 1} edges, got {edges.shape[0]}")
        if not np.isfinite(edges).all() or not np.all(np.diff(edges) > 0):
            raise ValueError(f"axis {a}: edges must be finite and strictly increasing")
        if int(col) != col or not 0 <= int(col) < values.shape[1]:
            raise ValueError(f"axis {a}: column {col} is out of range")
        cols.append(int(col))
        edge_list.append(edges)
    nb = [e.shape[0] - 1 for e in edge_list]
    pax, sizes = [], []
    for t, pan in enumerate(panels):
        ab = (int(pan), -1) if np.ndim(pan) == 0 else tuple(int(v) for v in pan)
        if len(ab) == 1:
            ab = (ab[0], -1)
        if len(ab) != 2 or not 0 <= ab[0] < len(axes) or not -1 <= ab[1] < len(axes):
            raise ValueError(f"panel {t}: axis index out of range")
        size = nb[ab[0]] * (nb[ab[1]] if ab[1] >= 0 else 1)
        if size > MAX_PANEL_BINS:
            raise ValueError(f"panel {t} has {size} bins: at most {MAX_PANEL_BINS}")
        pax.append(ab)
        sizes.append(size)
    return (values, np.concatenate(edge_list), np.array(cols, dtype=np.int32),
            np.concatenate([[0], np.cumsum([e.shape[0] for e in edge_list])]).astype(np.int64),
            np.array(pax, dtype=np.int32).reshape(-1, 2), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def _axis_bins(x, edges):
    """int64 [N]: the bin of every x on the axis, -1 outside."""
    j = np.searchsorted(edges, x, side="right") - 1
    j[x == edges[-1]] = edges.shape[0] - 2
    j[(x < edges[0]) | (x > edges[-1])] = -1
    return j.astype(np.int64)


def _entries(x, edges, axis_col, axis_start, panel_axes, panel_start):
    """int64 [P, N]: for every panel the flat entry of every merged row — its bin, or nbins + t for a row outside panel t."""
    nbins = int(panel_start[-1])
    per_axis = [_axis_bins(x[:, axis_col[a]], edges[axis_start[a]:axis_start[a + 1]]) for a in range(axis_col.shape[0])]
    out = np.empty((panel_axes.shape[0], x.shape[0]), np.int64)
    for t, (a, b) in enumerate(panel_axes):
        ja = per_axis[a]
        if b < 0:
            flat, inside = ja, ja >= 0
        else:
            jb = per_axis[b]
            flat, inside = ja * (axis_start[b + 1] - axis_start[b] - 1) + jb, (ja >= 0) & (jb >= 0)
        out[t] = np.where(inside, panel_start[t] + flat, nbins + t)
    return out


class _Welford:
    """The sequential update of the definition, vectorised over bins; NaN replicates are skipped."""

    def __init__(self, nbins):
        self.n, self.mean, self.m2 = np.zeros(nbins), np.zeros(nbins), np.zeros(nbins)
        self.min, self.max = np.full(nbins, np.inf), np.full(nbins, -np.inf)

    def add(self, x):
        if np.isnan(x).any():                                 # a replicate is NaN throughout or nowhere
            return
        self.n += 1.0
        d = x - self.mean
        self.mean += d / self.n
        self.m2 += d * (x - self.mean)
        self.min, self.max = np.minimum(self.min, x), np.maximum(self.max, x)

    def result(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            any_ = self.n > 0
            return tuple(np.where(any_, v, np.nan) for v in (self.mean, np.sqrt(self.m2 / self.n), self.min, self.max))


def _definition(values, logl, birth, run_start, flat, nsamples, code, bootstrap, seed, return_replicates):
    edges, axis_col, axis_start, panel_axes, panel_start = flat
    lay = merge._layout(logl, birth, run_start)
    N, R, P, nbins = logl.shape[0], lay["R"], panel_axes.shape[0], int(panel_start[-1])
    ent = _entries(values[lay["order"]], edges, axis_col, axis_start, panel_axes, panel_start)
    cnt = sum(np.bincount(ent[t], minlength=nbins + P) for t in range(P)).astype(np.int64)
    seeds = replicate_seeds(seed, nsamples)
    logz, info = np.empty(nsamples), np.empty(nsamples)
    mass = np.empty((nsamples, nbins)) if return_replicates else None
    outside = np.empty((nsamples, P)) if return_replicates else None
    acc = _Welford(nbins)
    step = max(1, _BLOCK_ELEMS // N)
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        w = merge.bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, _ = merge._block(lay, w, seeds[s0:s1], code == _abi.SHRINK_EXPECTED)
        for s in range(s0, s1):
            with np.errstate(invalid="ignore"):
                p = np.exp(logw[s - s0] - logz[s])
            m = np.rint(np.where(p > 0.0, p, 0.0) * SCALE).astype(np.int64)
            M = int(m.sum(dtype=np.int64))
            h = np.zeros(nbins + P, np.int64)
            rows = np.flatnonzero(m)                          # a row with m = 0 adds nothing
            mr = m[rows]
            for t in range(P):
                np.add.at(h, ent[t, rows], mr)
            with np.errstate(invalid="ignore", divide="ignore"):
                x = h.astype(np.float64) / np.float64(M) if M else np.full(nbins + P, np.nan)
            acc.add(x[:nbins])
            if return_replicates:
                mass[s], outside[s] = x[:nbins], x[nbins:]
    return logz, info, cnt[:nbins], cnt[nbins:], acc.result(), mass, outside


def _device(values, logl, birth, run_start, flat, nsamples, code, bootstrap, seed, return_replicates, device, block_bytes, timing):
    edges, axis_col, axis_start, panel_axes, panel_start = flat
    lib = _abi.load()
    N, R, P, nbins = logl.shape[0], run_start.shape[0] - 1, panel_axes.shape[0], int(panel_start[-1])
    logz, info = np.empty(nsamples), np.empty(nsamples)
    counts, outside_count, stats = np.empty(nbins, np.int64), np.empty(P, np.int64), np.empty((4, nbins))
    mass = np.empty((nsamples, nbins)) if return_replicates else None
    outside = np.empty((nsamples, P)) if return_replicates else None
    pax = np.ascontiguousarray(panel_axes)
    t = _abi.MarginalTiming()
    _abi.check(lib.rvll_marginal_replicates(
        int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(_i64p), R, _abi.as_dp(values),
        values.shape[1], _abi.as_dp(edges), _abi.as_ip(axis_col), axis_start.ctypes.data_as(_i64p), axis_col.shape[0],
        _abi.as_ip(pax), P, nsamples, code, 1 if bootstrap else 0, int(seed) & _M64, _abi.as_dp(logz), _abi.as_dp(info),
        counts.ctypes.data_as(_i64p), outside_count.ctypes.data_as(_i64p), _abi.as_dp(stats),
        _abi.as_dp(mass) if return_replicates else None, _abi.as_dp(outside) if return_replicates else None,
        int(block_bytes or 0), C.byref(t)))
    if timing is not None:
        timing.update({name: getattr(t, name) for name, _ in t._fields_})
    return logz, info, counts, outside_count, tuple(stats), mass, outside


def marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=1000, seed=0, mode="random", bootstrap=True,
                     device=None, return_replicates=False, block_bytes=None, timing=None):
    """Histograms of `values` (float64 [N, C] in input row order, finite, 1 <= C <= 64) over nsamples replicates of the merged run
    of the runs (logl, birth, run_start) as merge.replicates_arrays takes them.  axes: a list of (column, edges); panels: a list
    of axis indexes (1-D) or pairs of them (2-D).  A dict with counts [nbins] and outside_count [P] (int64), mean, std, min, max
    [nbins] (the statistics of the mass of every bin over the replicates), panel_start [P + 1], logz [S], information [S] and,
    with return_replicates, mass [S, nbins] and outside [S, P].  device=None evaluates the numpy definition, in blocks of
    replicates; device=k runs rvll_marginal_replicates on device k (block_bytes bounds table_bytes(N, A) plus a block of
    replicates of replicate_bytes(N, nbins, P) each; default: the table plus 8 GiB, of which no more than nsamples replicates
    are allocated; timing: a dict that receives the call's rvll_marginal_timing)."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    values, *flat = check_args(values, logl, axes, panels)
    fn = _definition if device is None else _device
    extra = () if device is None else (device, block_bytes, timing)
    logz, info, counts, outside_count, (mean, std, mn, mx), mass, outside = fn(
        values, logl, birth, run_start, flat, nsamples, code, bootstrap, seed, return_replicates, *extra)
    out = dict(counts=counts, outside_count=outside_count, mean=mean, std=std, min=mn, max=mx, panel_start=flat[4], logz=logz,
               information=info)
    if return_replicates:
        out.update(mass=mass, outside=outside)
    return out


def _edges(lo, hi, bins, log):
    if not hi > lo:                                           # a constant column: one unit of width about its value
        half = 0.5 * max(abs(lo) * 1e-6, 1e-12)
        lo, hi = lo - half, hi + half
    if log and lo > 0.0:
        edges = np.exp(np.linspace(np.log(lo), np.log(hi), bins + 1))
        edges[0], edges[-1] = lo, hi
        return edges
    return np.linspace(lo, hi, bins + 1)


def marginals(results, parnames, columns=None, derived=None, derived_names=(), order=False, bins=40, bins2d=None, corner=True,
              log_columns=None, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, block_bytes=None, timing=None):
    """The histograms of the reference's post-processing plots for finished runs (a list of NestedResult with samples and
    logl_birth), with error bars.  The columns are chosen as posterior.table chooses them (columns, derived with derived_names,
    order=True for the period ordering of the planets).  Every column gets a 1-D panel of `bins` bins and, with corner=True,
    every pair of columns a 2-D panel of bins2d x bins2d (default min(bins, 64)).  Edges span the [1e-4, 1 - 1e-4] quantile
    range of the column in the expected-weight run, linearly, or logarithmically for log_columns (default: the names containing
    "period", as in the reference's plots).  A dict: names; panels, a list with one dict a panel — columns (a tuple of names),
    edges (a tuple of arrays), counts, density (the expected weights, one replicate, no bootstrap: mass over the bin's width or
    area), density_err, density_min, density_max (the standard deviation, minimum and maximum over nsamples replicates with
    mode / bootstrap / seed), mass and mass_err (the same before the division), outside (the point mass outside the panel), 2-D
    arrays shaped [bins of the first column, bins of the second]; logz, logz_err, nsamples and replicates (marginals_arrays'
    dict)."""
    _, cols, logl, birth, run_start = posterior._values(results, columns, derived, order, parnames)
    names = list(parnames) if columns is None else [c if isinstance(c, str) else list(parnames)[int(c)] for c in columns]
    names += list(derived_names)
    ncols = cols.shape[1]
    if len(names) != ncols:
        raise ValueError(f"{ncols} columns but {len(names)} names (derived_names must name every derived column)")
    logs = [n for n in names if "period" in n] if log_columns is None else list(log_columns)
    bins2d = min(int(bins), 64) if bins2d is None else int(bins2d)
    rng = posterior.summarize_arrays(cols, logl, birth, run_start, RANGE_QUANTILES, 1, seed, "expected", False, device,
                                     block_bytes)["quantiles"][0]
    axes = [(c, _edges(rng[0, c], rng[1, c], int(bins), names[c] in logs)) for c in range(ncols)]
    panels = list(range(ncols))
    if corner:
        first2d = len(axes) if bins2d != int(bins) else 0
        if first2d:
            axes += [(c, _edges(rng[0, c], rng[1, c], bins2d, names[c] in logs)) for c in range(ncols)]
        panels += [(first2d + a, first2d + b) for a in range(ncols) for b in range(a + 1, ncols)]
    point = marginals_arrays(cols, logl, birth, run_start, axes, panels, 1, seed, "expected", False, device, True, block_bytes)
    reps = marginals_arrays(cols, logl, birth, run_start, axes, panels, nsamples, seed, mode, bootstrap, device, False,
                            block_bytes, timing)
    start = reps["panel_start"]
    out_panels = []
    for t, pan in enumerate(panels):
        ax = (pan,) if isinstance(pan, int) else pan
        edges = tuple(axes[a][1] for a in ax)
        shape = tuple(e.shape[0] - 1 for e in edges)
        size = np.diff(edges[0]) if len(ax) == 1 else np.outer(np.diff(edges[0]), np.diff(edges[1]))
        sl = slice(int(start[t]), int(start[t + 1]))
        mass = point["mass"][0, sl].reshape(shape)
        out_panels.append(dict(columns=tuple(names[axes[a][0]] for a in ax), edges=edges, counts=reps["counts"][sl].reshape(shape),
                               mass=mass, mass_err=reps["std"][sl].reshape(shape), density=mass / size,
                               density_err=reps["std"][sl].reshape(shape) / size, density_min=reps["min"][sl].reshape(shape) / size,
                               density_max=reps["max"][sl].reshape(shape) / size, outside=float(point["outside"][0, t])))
    return dict(names=names, panels=out_panels, nsamples=int(nsamples), logz=float(point["logz"][0]),
                logz_err=float(np.std(reps["logz"])), replicates=reps)


def credible_levels(mass2d, levels=(0.393, 0.865)):
    """The thresholds of a corner plot's contours: for every level the largest value v of mass2d (the mass or, over equal bins,
    the density of every bin; any shape) such that the bins with mass2d >= v hold at least that fraction of the total.  The
    defaults are the 1 and 2 sigma contours of a 2-D Gaussian, 1 - exp(-1/2) and 1 - exp(-2).  Host only."""
    m = np.sort(np.asarray(mass2d, dtype=np.float64).reshape(-1))[::-1]
    levels = np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if m.size == 0 or not np.all(np.isfinite(m)) or np.any(m < 0) or not m.sum() > 0:
        raise ValueError("mass2d must hold finite, non-negative values with a positive sum")
    if not np.all((levels > 0.0) & (levels < 1.0)):
        raise ValueError("levels must lie in the open interval (0, 1)")
    cum = np.cumsum(m) / m.sum()
    return m[np.minimum(np.searchsorted(cum, levels, side="left"), m.size - 1)]
