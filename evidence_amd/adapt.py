"""Step-count adaptation of the slice walk by how far its walkers move ("move-distance", after UltraNest's
RegionSliceSampler(adaptive_nsteps='move-distance')): the numpy definition of DESIGN §4h, which the device entry
(GpuRVModel.walk_distances_runs, rvll_walk_distances_runs in csrc/rvll_adapt.hip) reproduces.

Per iteration of a run every walker walks in a group g: the whole run when unclustered, the cluster of its start row when
clustered.  The group has the lower-triangular factor L_g its walk was whitened with, and member rows S_g: the survivors of
the iteration in that group.  All rows are unit-cube rows.

    delta(a, b)   = b - a componentwise; on wrapped dimensions the minimum image x - floor(x + 0.5)
    dist_g(a, b)  = sqrt(sum_k z_k z_k),  L_g z = delta(a, b) by forward substitution:
                    z_k = (delta_k - sum_{j<k} L_kj z_j) / L_kk, the inner sum in increasing j (s = 0; s = s + L_kj z_j),
                    the squares summed in increasing k, every operation rounded on its own
    pair_g        = the mean of dist_g over the unordered pairs of S_g (NaN when |S_g| < 2)
    move_w        = dist_g(start_w, end_w)

A walker is counted when its group's pair_g is defined, and far when move_w > pair_g.  With c counted and f far walkers in a
run's iteration, the next iteration's step count follows from this one's (`next_nsteps`): longer by a tenth (at least 1, at
most max_nsteps) when 2 f < c, shorter by a tenth (at least 1, never below min_nsteps) when 4 f >= 3 c, unchanged otherwise or
when c = 0.  Integers only, no random draws: a run with min_nsteps == max_nsteps == nsteps is the non-adaptive run bit for
bit.  `move` and every pair distance of the device are these bits; `pair` is within round-off of the mean (its summation
order is free).
"""
import numpy as np

MODES = ("move-distance",)
MAX_NSTEPS = 1000                     # the default ceiling of an adaptive run
_BLOCK_PAIRS = 1 << 16                # pairs the definition forms at a time


def dist(a, b, factor, wrapped=None):
    """dist [n] between the rows of a and b ([n, ndim] each) under the lower-triangular factor [ndim, ndim]."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    factor = np.asarray(factor, dtype=np.float64)
    n, D = a.shape
    delta = b - a
    if wrapped is not None:
        wd = np.flatnonzero(np.asarray(wrapped, dtype=bool).reshape(D))
        delta[:, wd] = delta[:, wd] - np.floor(delta[:, wd] + 0.5)
    z = np.empty((n, D))
    acc = np.zeros(n)
    for k in range(D):
        s = np.zeros(n)
        for j in range(k):
            s = s + factor[k, j] * z[:, j]
        z[:, k] = (delta[:, k] - s) / factor[k, k]
        acc = acc + z[:, k] * z[:, k]
    return np.sqrt(acc)


def pair_mean(rows, factor, wrapped=None):
    """pair_g: the mean of dist over the unordered pairs of rows [n, ndim]; NaN when n < 2."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[0]
    if n < 2:
        return float("nan")
    ii, jj = np.triu_indices(n, 1)
    total = 0.0
    for p0 in range(0, ii.shape[0], _BLOCK_PAIRS):
        sl = slice(p0, p0 + _BLOCK_PAIRS)
        total += float(np.sum(dist(rows[ii[sl]], rows[jj[sl]], factor, wrapped)))
    return total / (n * (n - 1) // 2)


def check_args(survivors, group_start, factors, wrapped, starts, ends, walker_group):
    """The arguments of walk_distances_runs in canonical form; raises ValueError where rvll_walk_distances_runs returns
    RVLL_E_INVALID."""
    survivors = np.ascontiguousarray(survivors, dtype=np.float64)
    if survivors.ndim != 2:
        raise ValueError("survivors must be [rows, ndim]")
    D = survivors.shape[1]
    group_start = np.ascontiguousarray(group_start, dtype=np.int64).reshape(-1)
    G = group_start.shape[0] - 1
    if G < 0 or group_start[0] != 0 or group_start[-1] != survivors.shape[0] or np.any(np.diff(group_start) < 0):
        raise ValueError("group_start must rise from 0 to the number of survivors")
    factors = np.ascontiguousarray(factors, dtype=np.float64)
    if factors.size != G * D * D:
        raise ValueError("factors must be [groups, ndim, ndim]")
    factors = factors.reshape(G, D, D)
    starts = np.ascontiguousarray(starts, dtype=np.float64).reshape(-1, D)
    ends = np.ascontiguousarray(ends, dtype=np.float64).reshape(-1, D)
    walker_group = np.ascontiguousarray(walker_group, dtype=np.int32).reshape(-1)
    if starts.shape != ends.shape or walker_group.shape[0] != starts.shape[0]:
        raise ValueError("starts, ends and walker_group must describe the same walkers")
    if walker_group.size and (walker_group.min() < 0 or walker_group.max() >= G):
        raise ValueError("walker_group out of range")
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool).reshape(D)
    return survivors, group_start, factors, wrapped, starts, ends, walker_group


def walk_distances_runs(survivors, group_start, factors, wrapped, starts, ends, walker_group):
    """G groups in one call: rows group_start[g] .. group_start[g + 1] of survivors are S_g, factors[g] is L_g; walker k walked
    from starts[k] to ends[k] in group walker_group[k].  Returns (pair [G], move [K])."""
    survivors, group_start, factors, wrapped, starts, ends, walker_group = check_args(
        survivors, group_start, factors, wrapped, starts, ends, walker_group)
    G = group_start.shape[0] - 1
    pair = np.array([pair_mean(survivors[group_start[g]:group_start[g + 1]], factors[g], wrapped) for g in range(G)])
    move = np.empty(starts.shape[0])
    for g in np.unique(walker_group):
        sel = np.flatnonzero(walker_group == g)
        move[sel] = dist(starts[sel], ends[sel], factors[g], wrapped)
    return pair, move


def far_counts(pair, move, walker_group, walker_run, nruns):
    """Per run: (counted [R], far [R]) — walker k of run walker_run[k] is counted when pair[walker_group[k]] is defined, far
    when move[k] > that pair."""
    pw = np.asarray(pair, dtype=np.float64)[np.asarray(walker_group, dtype=np.intp)]
    counted = ~np.isnan(pw)
    far = counted & (np.asarray(move, dtype=np.float64) > pw)
    run = np.asarray(walker_run, dtype=np.intp)
    return (np.bincount(run[counted], minlength=nruns).astype(np.int64),
            np.bincount(run[far], minlength=nruns).astype(np.int64))


def next_nsteps(n, far, counted, min_nsteps, max_nsteps):
    """The rule: the next iteration's step count from this one's n, with f far walkers of c counted.  Scalars or arrays."""
    n = np.asarray(n, dtype=np.int64)
    f = np.asarray(far, dtype=np.int64)
    c = np.asarray(counted, dtype=np.int64)
    step = np.maximum(1, n // 10)
    up = np.minimum(max_nsteps, n + step)
    down = np.maximum(min_nsteps, n - step)
    out = np.where(c == 0, n, np.where(2 * f < c, up, np.where(4 * f >= 3 * c, down, n)))
    return int(out) if out.ndim == 0 else out


def far_fraction(far, counted):
    """f / c per run (NaN where c = 0)."""
    f = np.asarray(far, dtype=np.float64)
    c = np.asarray(counted, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0, f / np.where(c > 0, c, 1.0), np.nan)


def check_settings(adaptive_nsteps, nsteps, min_nsteps, max_nsteps):
    """(min_nsteps, max_nsteps) of an adaptive run in canonical form (min_nsteps defaults to nsteps, max_nsteps to
    MAX_NSTEPS); ValueError on an unknown mode or a start outside [min_nsteps, max_nsteps]."""
    if adaptive_nsteps not in MODES:
        raise ValueError(f"adaptive_nsteps must be None or one of {MODES}")
    lo = int(nsteps if min_nsteps is None else min_nsteps)
    hi = int(MAX_NSTEPS if max_nsteps is None else max_nsteps)
    if not 1 <= lo <= int(nsteps) <= hi:
        raise ValueError("need 1 <= min_nsteps <= nsteps <= max_nsteps")
    return lo, hi
