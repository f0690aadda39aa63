"""MLFriends clustering of live points (Buchner 2016, 2019), in numpy: the reference implementation of the definition in
DESIGN §4e, which the device clusterer (GpuRVModel.cluster_runs, rvll_cluster_runs) reproduces bit for bit, and the default
clusterer of nested.run_nested_slice / run_nested_ensemble(clustering=True) on the host.

    cluster_runs(cube, run_start, scale, wrapped=None, nboot=30, seeds=()) -> (labels, nclusters, radius2)

Rows run_start[r] .. run_start[r + 1] of cube are run r.  Within a run, rows i and j are linked when their scaled distance
d2(i, j) (sum over dimensions in ascending order of ((u_i - u_j) wrapped) * scale)^2, every operation rounded on its own) is at
most the run's radius2; the clusters are the connected components, labelled 0, 1, ... in the order of their smallest row.
radius2 is the largest, over the half-split bootstraps b < nboot that leave at least one row in and one row out, of the
largest distance from a left-out row to its nearest kept row (row i is kept in bootstrap b when bit 63 - b of the splitmix64
word of (seeds[r], i) is set — the word rvll_math.h's uniform01 forms before its shift); without such a bootstrap, the
largest nearest-neighbour distance.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

MAX_BOOT = 32
_BLOCK_ELEMS = 1 << 22              # pair distances a block of rows holds at a time (32 MiB of doubles)


def keep_words(seed, n):
    """The splitmix64 words of (seed, 0 .. n-1) as uniform01 forms them, before its shift: uint64 [n]."""
    with np.errstate(over="ignore"):
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def kept_mask(seed, n, nboot):
    """bool [n, nboot]: row i is in bootstrap b."""
    z = keep_words(seed, n)
    shifts = np.uint64(63) - np.arange(nboot, dtype=np.uint64)
    return ((z[:, None] >> shifts[None, :]) & np.uint64(1)).astype(bool)


def pair_d2(a, b, scale, wrapped):
    """d2 [len(a), len(b)] in the definition's order of operations: per dimension, ascending, delta (wrapped: minus its
    round-half-even), times the scale, squared, added."""
    acc = np.zeros((a.shape[0], b.shape[0]))
    for d in range(a.shape[1]):
        delta = a[:, d, None] - b[None, :, d]
        if wrapped is not None and wrapped[d]:
            delta = delta - np.rint(delta)
        t = delta * scale[d]
        acc = acc + t * t
    return acc


def _blocks(n):
    step = max(1, _BLOCK_ELEMS // max(1, n))
    for i0 in range(0, n, step):
        yield i0, min(n, i0 + step)


def cluster_one(u, scale, wrapped=None, nboot=30, seed=0):
    """One run: (labels [n] int32, nclusters, radius2)."""
    n = u.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int32), 0, 0.0
    if n == 1:
        return np.zeros(1, dtype=np.int32), 1, 0.0
    kept = kept_mask(seed, n, nboot)
    qual = kept.any(axis=0) & (~kept).any(axis=0)
    rho = np.zeros(nboot)
    nn = 0.0
    for i0, i1 in _blocks(n):
        d2 = pair_d2(u[i0:i1], u, scale, wrapped)
        own = d2[np.arange(i1 - i0), np.arange(i0, i1)].copy()
        d2[np.arange(i1 - i0), np.arange(i0, i1)] = np.inf
        nn = max(nn, float(d2.min(axis=1).max()))
        d2[np.arange(i1 - i0), np.arange(i0, i1)] = own
        for b in np.flatnonzero(qual):
            left = np.flatnonzero(~kept[i0:i1, b])
            if left.size:
                rho[b] = max(rho[b], float(d2[np.ix_(left, np.flatnonzero(kept[:, b]))].min(axis=1).max()))
    radius2 = float(rho[qual].max()) if qual.any() else nn
    rows, cols = [], []
    for i0, i1 in _blocks(n):
        d2 = pair_d2(u[i0:i1], u, scale, wrapped)
        ii, jj = np.nonzero(d2 <= radius2)
        ii += i0
        upper = jj > ii
        rows.append(ii[upper]); cols.append(jj[upper])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    graph = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(n, n))
    ncl, comp = connected_components(graph, directed=False)
    _, first = np.unique(comp, return_index=True)           # each component's smallest row
    rank = np.empty(ncl, dtype=np.int32)
    rank[np.argsort(first)] = np.arange(ncl, dtype=np.int32)
    return rank[comp].astype(np.int32), int(ncl), radius2


def check_args(cube, run_start, scale, wrapped, nboot, seeds):
    """The arguments in canonical form: cube [N, D] float64, run_start int64 [R + 1], scale [R, D], wrapped bool [D] or None,
    nboot, seeds uint64 [R].  Raises ValueError where rvll_cluster_runs returns RVLL_E_INVALID."""
    cube = np.ascontiguousarray(cube, dtype=np.float64)
    if cube.ndim != 2:
        raise ValueError("cube must be [rows, ndim]")
    D = cube.shape[1]
    run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
    R = run_start.shape[0] - 1
    if R < 0 or run_start[0] != 0 or run_start[-1] != cube.shape[0] or np.any(np.diff(run_start) < 0):
        raise ValueError("run_start must rise from 0 to the number of rows")
    scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(R, D) if R else np.zeros((0, D))
    if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
        raise ValueError("scale must be finite and positive")
    if not 0 <= int(nboot) <= MAX_BOOT:
        raise ValueError(f"nboot must be in [0, {MAX_BOOT}]")
    seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
    if seeds.shape[0] != R:
        raise ValueError("seeds needs one entry per run")
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool).reshape(D)
    return cube, run_start, scale, wrapped, int(nboot), seeds


def cluster_runs(cube, run_start, scale, wrapped=None, nboot=30, seeds=()):
    """R independent row sets in one call: (labels [N] int32, nclusters [R] int32, radius2 [R] float64)."""
    cube, run_start, scale, wrapped, nboot, seeds = check_args(cube, run_start, scale, wrapped, nboot, seeds)
    R = run_start.shape[0] - 1
    labels = np.zeros(cube.shape[0], dtype=np.int32)
    nclusters = np.zeros(R, dtype=np.int32)
    radius2 = np.zeros(R)
    for r in range(R):
        a, b = run_start[r], run_start[r + 1]
        labels[a:b], nclusters[r], radius2[r] = cluster_one(cube[a:b], scale[r], wrapped, nboot, int(seeds[r]))
    return labels, nclusters, radius2
