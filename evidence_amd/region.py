"""MLFriends region sampling (Buchner 2016, 2019) as a nested-sampling proposal, in numpy: the definition that the
device entry (GpuRVModel.region_draw_runs, rvll_region_draw_runs, csrc/rvll_region.hip) follows, and the default region sampler
of nested.run_nested_slice / run_nested_ensemble(proposal="region") on the host.

    draw_runs(survivors, run_start, scale, radius2, lstar, seeds, kdraw, evaluate, wrapped=None, ...)
        -> (cube [R, kdraw, D], theta [R, kdraw, D], logl [R, kdraw], nfound [R], ncalls [R])   (+ the trace with trace=True)

Run r has m survivors u (rows run_start[r] .. run_start[r + 1] of `survivors`: unit-cube rows in rank order), the metric scale[r]
and radius2[r] as clustering.cluster_runs returns them, a contour lstar[r] and a seed.  Its region is the union of the balls
{x : pair_d2(x, u_j) <= radius2} around its survivors.  Candidates are numbered c = first, first + 1, ...; every random number of
candidate c is merge.uniform_at(seed, c << 8 | draw) (rvll_math.h's uniform01), so a candidate never depends on how many
candidates a call, a block or a launch handles.  Draws: 2 k and 2 k + 1 for the normal of dimension k, CENTRE, RADIUS, THIN.

Candidate c:
  1. centre    i = min(floor(U_CENTRE m), m - 1);
  2. offset    D normals g (the walk's Box-Muller, cosine branch), |g| = sqrt of the sum of g_k g_k in ascending k,
               rho = U_RADIUS ** (1 / D), f = sqrt(radius2) rho / |g|, cand_k = u_ik + (f g_k) / scale_k;
               a wrapped dimension is folded (x - floor(x), and 0 where that rounds to 1); any other dimension outside [0, 1)
               ends the candidate with the flag OUTSIDE;
  3. thinning  n = #{j : pair_d2(cand, u_j) <= radius2} (clustering.pair_d2's order of operations: + - * and rint only, exact
               on both sides); n = 0 (rounding alone can do that) ends the candidate with the flag LOST; it is kept iff
               U_THIN n < 1: a point inside n balls is proposed n times as often as a point inside one;
  4. log-L     kept candidates go through `evaluate` (cube -> theta, log-L); accepted iff log-L > lstar.
The run's new points are its first kdraw accepted candidates in candidate order; ncalls is the number of kept candidates up to
and including the last one taken (all kept ones when the run stays short within max_candidates: nfound < kdraw).  A run whose
ball meets its own image in a wrapped dimension (sqrt(radius2) / scale_k >= 0.5) would count such points twice: it draws
nothing (nfound = 0, ncalls = 0), and so does a run without survivors.

An accepted point is an exact, independent draw from the prior inside the contour wherever the region covers the contour.
"""
import numpy as np

from .clustering import pair_d2
from .merge import uniform_at

OUTSIDE, LOST, KEPT, ACCEPTED = 1, 2, 4, 8        # trace flags of a candidate
CENTRE, RADIUS, THIN = 128, 129, 130              # draw numbers next to the normals' 2 k, 2 k + 1 (k < 64)
MAX_DIMS = 64
TWO_PI = 6.283185307179586
DEFAULT_MAX_CANDIDATES = 1 << 18                  # per run and call (DESIGN §4n says how it was chosen)
DEFAULT_BLOCK = 4096                              # candidates a run proposes at a time


def counters(c, draw):
    """uint64: the counter of draw `draw` of candidate c."""
    return (np.asarray(c, dtype=np.uint64) << np.uint64(8)) | np.asarray(draw, dtype=np.uint64)


def normal_at(seed, ctr):
    """rvll_tile.h's walk_normal in float64: Box-Muller, cosine branch, on the uniforms of counters ctr and ctr + 1."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    u1, u2 = uniform_at(seed, ctr), uniform_at(seed, ctr + np.uint64(1))
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)


def blocked(scale, radius2, wrapped):
    """A run whose ball meets its own image in a wrapped dimension draws nothing."""
    if wrapped is None or not np.any(wrapped):
        return False
    return bool(np.any(np.sqrt(radius2) / np.asarray(scale)[np.asarray(wrapped, dtype=bool)] >= 0.5))


def candidates(u, scale, radius2, seed, c, wrapped=None):
    """Steps 1 and 2 for the candidates c (uint64 [n]) of one run: (cand [n, D], outside [n] bool)."""
    m, D = u.shape
    seed = np.uint64(int(seed) & (2 ** 64 - 1))
    c = np.asarray(c, dtype=np.uint64)
    i = np.minimum(np.floor(uniform_at(seed, counters(c, CENTRE)) * float(m)), float(m - 1)).astype(np.intp)
    g = normal_at(seed, counters(c[:, None], 2 * np.arange(D, dtype=np.uint64)[None, :]))
    norm2 = np.zeros(c.shape[0])
    for k in range(D):
        norm2 = norm2 + g[:, k] * g[:, k]
    rho = uniform_at(seed, counters(c, RADIUS)) ** (1.0 / float(D))
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sqrt(radius2) * rho / np.sqrt(norm2)
        cand = u[i] + (f[:, None] * g) / np.asarray(scale)[None, :]
        outside = np.zeros(c.shape[0], dtype=bool)
        for k in range(D):
            if wrapped is not None and wrapped[k]:
                w = cand[:, k] - np.floor(cand[:, k])
                cand[:, k] = np.where(w >= 1.0, 0.0, w)
            else:
                outside |= ~((cand[:, k] >= 0.0) & (cand[:, k] < 1.0))
    return cand, outside


def neighbours(cand, u, scale, radius2, wrapped=None):
    """n [len(cand)]: the survivors whose ball holds the candidate."""
    return np.count_nonzero(pair_d2(cand, u, scale, wrapped) <= radius2, axis=1).astype(np.int64)


def thin_keep(seed, c, n):
    """Step 3's decision: kept iff U_THIN n < 1 (a multiply, so that it is exact)."""
    seed = np.uint64(int(seed) & (2 ** 64 - 1))
    return (n > 0) & (uniform_at(seed, counters(c, THIN)) * n.astype(np.float64) < 1.0)


def select(kept, accepted, need):
    """The first `need` accepted candidates of a block in candidate order: (their indexes, calls) — calls counts the kept
    candidates up to and including the last one taken, all of them when fewer than `need` are accepted."""
    acc = np.flatnonzero(accepted)
    if acc.size >= need:
        acc = acc[:need]
        return acc, int(np.count_nonzero(kept[:acc[-1] + 1])) if need else 0
    return acc, int(np.count_nonzero(kept))


def check_args(survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped, first, max_candidates, block):
    """The arguments in canonical form.  Raises ValueError where rvll_region_draw_runs returns RVLL_E_INVALID / _UNSUPPORTED."""
    survivors = np.ascontiguousarray(survivors, dtype=np.float64)
    if survivors.ndim != 2:
        raise ValueError("survivors must be [rows, ndim]")
    D = survivors.shape[1]
    if not 1 <= D <= MAX_DIMS:
        raise ValueError(f"region sampling takes 1 .. {MAX_DIMS} parameters")
    run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
    R = run_start.shape[0] - 1
    if R < 0 or run_start[0] != 0 or run_start[-1] != survivors.shape[0] or np.any(np.diff(run_start) < 0):
        raise ValueError("run_start must rise from 0 to the number of rows")
    scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(R, D) if R else np.zeros((0, D))
    if not (np.all(np.isfinite(scale)) and np.all(scale > 0)):
        raise ValueError("scale must be finite and positive")
    radius2 = np.ascontiguousarray(radius2, dtype=np.float64).reshape(-1)
    if radius2.shape[0] != R or not (np.all(np.isfinite(radius2)) and np.all(radius2 >= 0)):
        raise ValueError("radius2 needs one finite, non-negative entry per run")
    lstar = np.ascontiguousarray(lstar, dtype=np.float64).reshape(-1)
    if lstar.shape[0] != R or np.any(np.isnan(lstar)):
        raise ValueError("lstar needs one entry per run, none NaN")
    seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
    if seeds.shape[0] != R:
        raise ValueError("seeds needs one entry per run")
    wrapped = None if wrapped is None else np.asarray(wrapped, dtype=bool).reshape(D)
    kdraw, first, max_candidates, block = int(kdraw), int(first), int(max_candidates), int(block)
    if kdraw < 0 or first < 0 or max_candidates < 0 or first + max_candidates >= 2 ** 55:
        raise ValueError("kdraw, first and max_candidates must not be negative (first + max_candidates below 2^55)")
    if not 1 <= block <= 1 << 20:
        raise ValueError("block must be in [1, 2^20]")
    return survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped, first, max_candidates, block


def draw_runs(survivors, run_start, scale, radius2, lstar, seeds, kdraw, evaluate, wrapped=None,
              max_candidates=DEFAULT_MAX_CANDIDATES, trace=False, first=0, block=DEFAULT_BLOCK):
    """kdraw region draws of every run (the module's docstring has the definition).  evaluate(cube [n, D]) -> (theta, logl).
    Candidates first .. first + max_candidates - 1 are available to every run; a run proposes `block` of them at a time until
    it has its kdraw points (the results do not depend on block; the length of the trace does).
    Returns (cube [R, kdraw, D], theta [R, kdraw, D], logl [R, kdraw], nfound [R] int32, ncalls [R] int64), rows past nfound
    NaN; with trace=True also a list of R dicts over every candidate the run evaluated, in candidate order:
    c (uint64), cube [n, D], flags (OUTSIDE | LOST | KEPT | ACCEPTED), n (0 where OUTSIDE), logl (NaN where not kept)."""
    survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped, first, max_candidates, block = check_args(
        survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped, first, max_candidates, block)
    R, D = run_start.shape[0] - 1, survivors.shape[1]
    cube = np.full((R, kdraw, D), np.nan)
    theta = np.full((R, kdraw, D), np.nan)
    logl = np.full((R, kdraw), np.nan)
    nfound = np.zeros(R, dtype=np.int32)
    ncalls = np.zeros(R, dtype=np.int64)
    traces = []
    for r in range(R):
        u = survivors[run_start[r]:run_start[r + 1]]
        tr = {"c": [], "cube": [], "flags": [], "n": [], "logl": []}
        c0, cend = first, first + max_candidates
        active = len(u) > 0 and not blocked(scale[r], radius2[r], wrapped)
        while active and nfound[r] < kdraw and c0 < cend:
            c = np.arange(c0, min(c0 + block, cend), dtype=np.uint64)
            c0 += block
            cand, outside = candidates(u, scale[r], radius2[r], seeds[r], c, wrapped)
            n = np.zeros(c.shape[0], dtype=np.int64)
            inside = ~outside
            n[inside] = neighbours(cand[inside], u, scale[r], radius2[r], wrapped)
            kept = inside & thin_keep(seeds[r], c, n)
            flags = np.where(outside, OUTSIDE, np.where(n == 0, LOST, 0)).astype(np.int32)
            ll = np.full(c.shape[0], np.nan)
            th = np.full((c.shape[0], D), np.nan)
            if kept.any():
                t, l = evaluate(cand[kept])
                th[kept], ll[kept] = np.asarray(t, dtype=np.float64), np.asarray(l, dtype=np.float64)
            accepted = kept & (ll > lstar[r])
            flags |= np.where(kept, KEPT, 0).astype(np.int32) | np.where(accepted, ACCEPTED, 0).astype(np.int32)
            take, calls = select(kept, accepted, kdraw - int(nfound[r]))
            a, b = int(nfound[r]), int(nfound[r]) + take.size
            cube[r, a:b], theta[r, a:b], logl[r, a:b] = cand[take], th[take], ll[take]
            nfound[r] = b
            ncalls[r] += calls
            if trace:
                tr["c"].append(c); tr["cube"].append(cand); tr["flags"].append(flags); tr["n"].append(n); tr["logl"].append(ll)
        if trace:
            traces.append({"c": np.concatenate(tr["c"]) if tr["c"] else np.zeros(0, dtype=np.uint64),
                           "cube": np.concatenate(tr["cube"]) if tr["cube"] else np.zeros((0, D)),
                           "flags": np.concatenate(tr["flags"]) if tr["flags"] else np.zeros(0, dtype=np.int32),
                           "n": np.concatenate(tr["n"]) if tr["n"] else np.zeros(0, dtype=np.int64),
                           "logl": np.concatenate(tr["logl"]) if tr["logl"] else np.zeros(0)})
    if trace:
        return cube, theta, logl, nfound, ncalls, traces
    return cube, theta, logl, nfound, ncalls
