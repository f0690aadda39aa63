"""PolyChord-style stepping-out slice proposal: the numpy definition that run_nested_slice's host walk runs and
the device walk (rvll_set_walk_proposal(RVLL_PROPOSAL_STEPOUT), csrc/rvll_walk.hip) follows.

Move m of a walker with whitening factor L, start x0 (logL(x0) > lstar) and D = ndim parameters:
  1. direction d = L q_{m mod D}, q the rows of a random orthonormal basis drawn anew at every m mod D == 0 (modified
     Gram-Schmidt of D standard normals, gram_schmidt); d is NOT normalised: t is measured in whitened units;
  2. the wall chord [cmin, cmax] of t from the coordinates that are not wrapped (wall_chord); wrapped ones wrap mod 1;
  3. the bracket lo = -w v, hi = lo + w (v ~ U(0, 1)), each clamped to the wall chord; an end on the chord's limit is out;
  4. step out: while hi is not out and logL(x0 + hi d) > lstar, hi += w (clamped); then the same for lo;
  5. shrink: t = lo + (hi - lo) U until logL > lstar, moving lo or hi to a rejected t by its sign;
  6. expansions and shrink candidates count together against max_rounds; a move that reaches it stays at x0.
Every evaluated end and every shrink candidate is one likelihood call; ends clamped to a wall cost none.
"""
import numpy as np

PROPOSALS = ("chord", "stepout")


def check_proposal(proposal, step_width):
    """The proposal keywords of the drivers and walk methods, checked: returns (proposal, float(step_width))."""
    if proposal not in PROPOSALS:
        raise ValueError(f"proposal must be one of {PROPOSALS}, not {proposal!r}")
    w = float(step_width)
    if not (np.isfinite(w) and w > 0.0):
        raise ValueError("step_width must be positive and finite")
    return proposal, w


def gram_schmidt(g):
    """Modified Gram-Schmidt of the rows of g [..., D, D] in the written-out order: q_i = g_i, then for j < i ascending
    q_i -= (q_j . q_i) q_j, then q_i /= |q_i|.  Returns the orthonormal rows q (same shape)."""
    q = np.array(g, dtype=np.float64, copy=True)
    D = q.shape[-1]
    for i in range(D):
        for j in range(i):
            dot = np.sum(q[..., j, :] * q[..., i, :], axis=-1)
            q[..., i, :] -= dot[..., None] * q[..., j, :]
        q[..., i, :] /= np.sqrt(np.sum(q[..., i, :] * q[..., i, :], axis=-1))[..., None]
    return q


def wall_chord(u, d, wrapped):
    """Range [cmin, cmax] of t for which u + t d stays inside the cube's walls: nested._chord's operations over the
    coordinates that are not wrapped.  Wrapped coordinates set no limit (and no half-turn limit either: that one is
    centred on the walker, and an interval cut by a set that depends on x0 breaks reversibility)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (0.0 - u) / d
        t1 = (1.0 - u) / d
    lim = d != 0
    if wrapped is not None:
        lim = lim & ~np.asarray(wrapped, dtype=bool)
    lo = np.where(lim, np.minimum(t0, t1), -np.inf)
    hi = np.where(lim, np.maximum(t0, t1), np.inf)
    return lo.max(axis=1), hi.min(axis=1)


def walk(wu, wt, wl, lstar, factors, wrapped, nsteps, max_rounds, step_width, rng, evaluate):
    """nsteps stepping-out moves of every walker inside logL > lstar; wu / wt / wl [k, ndim] / [k, ndim] / [k] (unit-cube
    rows, theta, log-L) are updated in place.  factors: one [ndim, ndim] lower-triangular whitening factor, or one per
    walker [k, ndim, ndim].  evaluate(cand [n, ndim]) -> (theta, logl): one batched call per round, every unfinished
    walker's next candidate (an end of its bracket or a shrink point).  Draws from rng: the basis normals [k, D, D] at
    every m mod D == 0, v [k] once per move, one uniform per shrinking walker and round (in walker order).  Returns the
    likelihood calls."""
    k, D = wu.shape
    factors = np.asarray(factors, dtype=np.float64)
    many = factors.ndim == 3
    w = float(step_width)
    one_below = np.nextafter(1.0, 0.0)
    wr = None if wrapped is None else np.asarray(wrapped, dtype=bool)
    ncall = 0
    q = None
    for m in range(nsteps):
        if m % D == 0:
            q = gram_schmidt(rng.standard_normal((k, D, D)))
        z = q[:, m % D, :]
        d = np.einsum("kij,kj->ki", factors, z) if many else z @ factors.T
        cmin, cmax = wall_chord(wu, d, wr)
        v = rng.random(k)
        lo = np.maximum(-w * v, cmin)
        hi = np.minimum(-w * v + w, cmax)
        phase = np.where(hi < cmax, 0, np.where(lo > cmin, 1, 2))
        rounds = np.zeros(k, dtype=np.int64)
        todo = np.arange(k)
        while todo.size:
            ph = phase[todo]
            t = np.where(ph == 0, hi[todo], lo[todo])
            sh = ph == 2
            if sh.any():
                i = todo[sh]
                t[sh] = lo[i] + (hi[i] - lo[i]) * rng.random(i.size)
            cand = wu[todo] + t[:, None] * d[todo]
            if wr is not None:
                cand[:, wr] %= 1.0
            cand = np.clip(cand, 0.0, one_below)
            ct, cl = evaluate(cand)
            ct = np.asarray(ct, dtype=np.float64)
            cl = np.asarray(cl, dtype=np.float64)
            ncall += todo.size
            ok = cl > lstar
            acc = sh & ok                                              # accepted: the walker moves
            a = todo[acc]
            wu[a], wt[a], wl[a] = cand[acc], ct[acc], cl[acc]
            rej = sh & ~ok                                             # rejected shrink point: bracket towards t = 0
            neg = t < 0
            lo[todo[rej & neg]] = t[rej & neg]
            hi[todo[rej & ~neg]] = t[rej & ~neg]
            r0 = todo[ph == 0]                                         # right end: step out while inside
            inside = ok[ph == 0]
            hi[r0[inside]] = np.minimum(hi[r0[inside]] + w, cmax[r0[inside]])
            end = ~inside | ~(hi[r0] < cmax[r0])
            phase[r0[end]] = np.where(lo[r0[end]] > cmin[r0[end]], 1, 2)
            l0 = todo[ph == 1]                                         # then the left end
            inside = ok[ph == 1]
            lo[l0[inside]] = np.maximum(lo[l0[inside]] - w, cmin[l0[inside]])
            end = ~inside | ~(lo[l0] > cmin[l0])
            phase[l0[end]] = 2
            rounds[todo] += 1
            todo = todo[~acc & (rounds[todo] < max_rounds)]
    return ncall
