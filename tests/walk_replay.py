"""One move of the device proposal walk, replayed on the host from its documented counters (the header of
csrc/rvll_walk_kernel.h) — the reference the device walk is pinned to, move by move (test_gpu_walk_replay.py; checked itself,
without a GPU, by test_walk_replay_host.py).  Plain numpy, vectorised over walkers; no GPU, no ctypes.

Counters.  Every draw of walker `wid` is uniform01(seed, (wid << 32) | (move << 14) | draw) of rvll_math.h:

    proposal  value                              move field       draw field
    chord     normal z_k of move m               m                2 k  (and 2 k + 1: Box-Muller takes two uniforms)
    stepout   normal g_vk of basis b = m div D   b                2 (v D + k)  (and + 1)
    both      shrink candidate of round r        m                8192 + r      (r < max_rounds <= 4096)
    stepout   offset v of the bracket            m                12288

A move.  chord: d = L z / |L z|, [lo, hi] = nested._chord(u, d, wrapped); candidates t = lo + (hi - lo) U(8192 + r), a rejected
t moves lo if t < 0, else hi; at most max_rounds candidates, then the walker stays.  stepout: d = L q_{m mod D} (q =
Gram-Schmidt of the basis normals, d not normalised), [cmin, cmax] = stepout.wall_chord, bracket lo = max(-w v, cmin),
hi = min(-w v + w, cmax), phases right / left / shrink as stepout.py steps 3 - 6 (an end on the wall chord costs no call, shrink
round r draws U(8192 + r) with r counting the expansions too).  Candidate c = u + t d, wrapped coordinates c -= floor(c), clamp to
[0, nextafter(1, 0)], rounded to float64 for evaluate(cand) -> (theta, logl).

Precision.  dtype is the arithmetic's: numpy.longdouble is the reference, float64 measures how far rounding alone moves an end
point (the uniforms are exact in both).  Sums run in the kernel's order (ascending index), so the float64 replay differs from the
device only by fused multiply-adds and the device's own log / sincos.

Conditioning.  The rounding of an end row grows with two figures of the move itself, which the replay returns as their product
`scale` (>= 1): the largest |t d_k| of the accepted step where that is more than one — a stepout bracket has no half-turn
limit, so a wrapped coordinate may go round many times before c -= floor(c), and the rounding of t d_k is relative to the way gone,
not to where it ends — and, for stepout, the inverse of the smallest share Gram-Schmidt left of the normal vectors the
direction is built from (the projections' rounding is amplified by it, in any float64 evaluation and so in the device's).
An end row is compared within tol_u * scale: tol_u is the tolerance of a well-conditioned move (scale is 1 for a chord move
unless a wrapped coordinate's half turn is more than one, so there the bound is tol_u itself, under 1e-12).  The bound on a
cube coordinate never exceeds TOL_CEILING = 1e-8: a pair whose tol_u * scale would is "loose", left out of the end-row
comparison and counted with the fragile ones under the cap (its decisions and calls are still compared).

Fragile.  A move is fragile if a comparison it made came within a margin of flipping, judged on the replay's own values:
|logL - lstar| <= eps_l max(1, |lstar|) for an evaluated candidate or end, |t| <= eps_t for a rejected shrink candidate (its
sign picks the end), and for stepout an unclamped end of the bracket within eps_t of the wall chord's limit (the comparison
that decides whether the end is out).  Such (walker, move) pairs are left out of comparisons by the callers.
"""
from types import SimpleNamespace

import numpy as np

from evidence_amd import stepout
from evidence_amd.merge import uniform_at
from evidence_amd.nested import _chord

SHRINK_DRAW = 8192
OFFSET_DRAW = 12288
MAX_ROUNDS = 4096            # what the entry accepts (walk_check_args): max_rounds <= 4096, nsteps < 2^18, walker_base + K < 2^32
MAX_NSTEPS = 1 << 18
STEPOUT_MAX_NDIM = 64        # kStepoutMaxD
EPS_L = 1e-9
EPS_T = 1e-9
FRAGILE_CAP = 0.005
# the largest distance / scale between the float64 and the longdouble replay of one move's end row, over every non-fragile move
# of the cases of test_walk_replay_host.py (profiles/walk_replay.txt: 3.4e-13, a stepout walk with brackets 20 wide; 1.2e-14
# for chord walks), and the end-row tolerance of the device comparison.  The margin for what the float64 replay does not
# model (fused multiply-adds, the device's log / sincos) is 2, not 16: the spread is the tail of a conditioning effect (a short
# normal vector, a limiting coordinate with a small d_k), which the device — the same float64 operations in the same order —
# shares, and 16 times it would pass the ceiling of 1e-12 that a tolerance on a unit-cube coordinate has to stay under here.
SPREAD = 3.5e-13
TOL_U = 2 * SPREAD
TOL_CEILING = 1e-8           # no end row is compared more loosely than this, whatever its move's conditioning
_M64 = (1 << 64) - 1
ONE_BELOW = np.nextafter(1.0, 0.0)
TWO_PI = 2.0 * np.pi         # fl(2 pi): the device's kTwoPi


def counter(wid, move, draw):
    """uint64 (wid << 32) | (move << 14) | draw, elementwise."""
    return ((np.asarray(wid, dtype=np.uint64) << np.uint64(32)) | (np.asarray(move, dtype=np.uint64) << np.uint64(14))
            | np.asarray(draw, dtype=np.uint64))


def uniform(seed, ctr):
    """uniform01(seed, ctr) of rvll_math.h, bit for bit (merge.uniform_at)."""
    return uniform_at(np.asarray(seed, dtype=np.uint64), ctr)


def normal(seed, ctr, dtype=np.longdouble):
    """walk_normal: Box-Muller, cosine branch, on the uniforms of counters ctr and ctr + 1."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    u1 = uniform(seed, ctr).astype(dtype)
    u2 = uniform(seed, ctr + np.uint64(1)).astype(dtype)
    return np.sqrt(dtype(-2.0) * np.log(dtype(1.0) - u1)) * np.cos(dtype(TWO_PI) * u2)


def gram_schmidt(g, nvec=None, want_ratio=False):
    """stepout.gram_schmidt's operations in g's own dtype (that one computes in float64), sums in ascending index: rows
    0 .. nvec - 1 of the orthonormal basis of g [K, D, D].  want_ratio: also the smallest |residual of g_i| / |g_i| over those
    rows, per basis — what is left of a normal vector after the projections; rounding in them is amplified by its inverse."""
    q = np.array(g, copy=True)
    D = q.shape[-1]
    nvec = D if nvec is None else nvec
    ratio = np.ones(q.shape[0], dtype=q.dtype)
    for i in range(nvec):
        whole = np.sqrt(_dot(q[:, i, :], q[:, i, :]))
        for j in range(i):
            dot = _dot(q[:, j, :], q[:, i, :])
            q[:, i, :] -= dot[:, None] * q[:, j, :]
        left = np.sqrt(_dot(q[:, i, :], q[:, i, :]))
        q[:, i, :] /= left[:, None]
        ratio = np.minimum(ratio, left / whole)
    return (q[:, :nvec, :], ratio) if want_ratio else q[:, :nvec, :]


def _dot(a, b):
    acc = np.zeros(a.shape[0], dtype=a.dtype)
    for k in range(a.shape[1]):
        acc = acc + a[:, k] * b[:, k]
    return acc


def _whiten(chol, z):
    """L z for the lower-triangular factor(s) chol [D, D] or [K, D, D], row k summed over j = 0 .. k."""
    D = z.shape[1]
    out = np.zeros_like(z)
    for k in range(D):
        acc = np.zeros(z.shape[0], dtype=z.dtype)
        for j in range(k + 1):
            acc = acc + chol[..., k, j] * z[:, j]
        out[:, k] = acc
    return out


def candidate(u, t, d, wrapped):
    c = u + t[:, None] * d
    if wrapped is not None and wrapped.any():
        c[:, wrapped] -= np.floor(c[:, wrapped])
    return np.clip(c, 0.0, ONE_BELOW)


def circular_distance(a, b, wrapped):
    """max over coordinates of |a - b| (the shorter way round on wrapped coordinates), per row; in the wider dtype."""
    diff = np.abs(np.asarray(a) - np.asarray(b))
    if wrapped is not None and np.any(wrapped):
        wr = np.asarray(wrapped, dtype=bool)
        diff[:, wr] = np.minimum(diff[:, wr], 1.0 - diff[:, wr])
    return diff.max(axis=1) if diff.shape[1] else np.zeros(diff.shape[0])


def replay_move(u, theta, logl, move, *, proposal, seed, wid, lstar, chol, wrapped, max_rounds, evaluate, step_width=1.0,
                dtype=np.longdouble, eps_l=EPS_L, eps_t=EPS_T):
    """Move `move` (0-based) of the walkers at unit-cube rows u [K, D] (theta, logl: their float64 theta rows and log-L).
    seed, wid, lstar: scalars or one per walker; chol [D, D] or [K, D, D]; wrapped: bool [D] or None.  Returns a namespace of
    per-walker arrays: u (end row, dtype), theta, logl (float64; the start's where the walker stayed), calls (int64), moved,
    fragile (bool), scale (below: Conditioning), and d, lo, hi (the direction and the bracket the move ended with)."""
    if proposal not in stepout.PROPOSALS:
        raise ValueError(proposal)
    u0 = np.asarray(u, dtype=np.float64)
    K, D = u0.shape
    if not (1 <= max_rounds <= MAX_ROUNDS and 0 <= move < MAX_NSTEPS):
        raise ValueError("max_rounds / move out of the entry's range")
    if proposal == "stepout" and D > STEPOUT_MAX_NDIM:
        raise ValueError("a stepout walk takes at most 64 parameters")
    x = u0.astype(dtype)
    seed = np.broadcast_to(np.asarray(seed, dtype=np.uint64), (K,))
    wid = np.broadcast_to(np.asarray(wid, dtype=np.uint64), (K,))
    lstar = np.broadcast_to(np.asarray(lstar, dtype=np.float64), (K,))
    cf = np.asarray(chol, dtype=np.float64).astype(dtype)
    wr = None if wrapped is None else np.asarray(wrapped, dtype=bool)
    margin = eps_l * np.maximum(1.0, np.abs(lstar))
    cols = np.arange(D, dtype=np.uint64)
    w = dtype(step_width)

    out_u = x.copy()
    out_t = np.array(theta, dtype=np.float64, copy=True).reshape(K, -1)
    out_l = np.array(logl, dtype=np.float64, copy=True)
    calls = np.zeros(K, dtype=np.int64)
    moved = np.zeros(K, dtype=bool)
    fragile = np.zeros(K, dtype=bool)
    scale = np.ones(K)

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if proposal == "chord":
            z = normal(seed[:, None], counter(wid[:, None], move, 2 * cols[None, :]), dtype)
            d = _whiten(cf, z)
            d = d * (dtype(1.0) / np.sqrt(_dot(d, d)))[:, None]
            lo, hi = _chord(x, d, wr)
            phase = np.full(K, 2)
            cmin = cmax = None
        else:
            b, iv = divmod(int(move), D)
            draws = 2 * (np.arange(iv + 1, dtype=np.uint64)[:, None] * np.uint64(D) + cols[None, :])          # [iv + 1, D]
            g = normal(seed[:, None, None], counter(wid[:, None, None], b, draws[None, :, :]), dtype)
            g = np.concatenate([g, np.zeros((K, D - iv - 1, D), dtype=dtype)], axis=1)
            q, ratio = gram_schmidt(g, iv + 1, want_ratio=True)
            scale = (1.0 / ratio).astype(np.float64)
            d = _whiten(cf, q[:, iv, :])
            cmin, cmax = stepout.wall_chord(x, d, wr)
            v = uniform(seed, counter(wid, move, OFFSET_DRAW)).astype(dtype)
            blo = -w * v
            bhi = blo + w
            fragile |= (np.abs(blo - cmin) <= eps_t) | (np.abs(bhi - cmax) <= eps_t)
            lo, hi = np.maximum(blo, cmin), np.minimum(bhi, cmax)
            phase = np.where(hi < cmax, 0, np.where(lo > cmin, 1, 2))
        lo, hi = np.array(lo, dtype=dtype), np.array(hi, dtype=dtype)
        todo = np.arange(K)
        for r in range(max_rounds):
            if not todo.size:
                break
            ph = phase[todo]
            U = uniform(seed[todo], counter(wid[todo], move, SHRINK_DRAW + r)).astype(dtype)
            t = np.where(ph == 0, hi[todo], np.where(ph == 1, lo[todo], lo[todo] + (hi[todo] - lo[todo]) * U))
            cand = candidate(x[todo], t, d[todo], wr)
            ct, cl = evaluate(np.ascontiguousarray(cand.astype(np.float64)))
            ct = np.asarray(ct, dtype=np.float64).reshape(todo.size, -1)
            cl = np.asarray(cl, dtype=np.float64)
            calls[todo] += 1
            ok = cl > lstar[todo]
            fragile[todo] |= np.isfinite(lstar[todo]) & (np.abs(cl - lstar[todo]) <= margin[todo])
            sh = ph == 2
            acc = sh & ok
            a = todo[acc]
            out_u[a], out_t[a], out_l[a], moved[a] = cand[acc], ct[acc], cl[acc], True
            scale[a] *= np.maximum(1.0, np.abs(t[acc, None] * d[a]).max(axis=1).astype(np.float64))
            rej = sh & ~ok
            fragile[todo[rej]] |= np.abs(t[rej]) <= eps_t
            neg = t < 0
            lo[todo[rej & neg]] = t[rej & neg]
            hi[todo[rej & ~neg]] = t[rej & ~neg]
            if proposal == "stepout":
                for end, sign, lim in ((0, 1, cmax), (1, -1, cmin)):
                    i, inside = todo[ph == end], ok[ph == end]
                    cur = hi if end == 0 else lo
                    step = cur[i[inside]] + sign * w
                    fragile[i[inside]] |= np.abs(step - lim[i[inside]]) <= eps_t
                    cur[i[inside]] = np.minimum(step, lim[i[inside]]) if end == 0 else np.maximum(step, lim[i[inside]])
                    over = ~inside | ~((cur[i] < lim[i]) if end == 0 else (cur[i] > lim[i]))
                    phase[i[over]] = np.where(lo[i[over]] > cmin[i[over]], 1, 2) if end == 0 else 2
            todo = todo[~acc]
    return SimpleNamespace(u=out_u, theta=out_t, logl=out_l, calls=calls, moved=moved, fragile=fragile, scale=scale, d=d, lo=lo, hi=hi)


def walk(u, theta, logl, nsteps, dtype=np.float64, **kw):
    """nsteps replayed moves from (u, theta, logl), the rows rounded to float64 after every move as the device stores them.
    Returns (states, ncalls, fragile): states[n] = (u, theta, logl) after n moves, ncalls[n] the calls so far, fragile
    [nsteps, K]."""
    state = (np.array(u, dtype=np.float64), np.array(theta, dtype=np.float64), np.array(logl, dtype=np.float64))
    states, ncalls, fragile = [state], [0], []
    for m in range(nsteps):
        r = replay_move(*state, m, dtype=dtype, **kw)
        state = (r.u.astype(np.float64), r.theta, r.logl)
        states.append(state)
        ncalls.append(ncalls[-1] + int(r.calls.sum()))
        fragile.append(r.fragile)
    return states, ncalls, np.array(fragile).reshape(nsteps, -1)


def check_prefixes(states, ncalls, evaluate, *, tol_u, wrapped, groups=None, steps=None, **walk):
    """The comparison of test_gpu_walk_replay.py.  states[n] = (u, theta, logl) of the walk under test after n moves
    (n = 0 .. N, float64), ncalls[n] its call total (a scalar, or one per group with groups [K] naming each walker's);
    steps: moves per group if they differ (a walker whose group makes s moves does not change after prefix s).  walk: the
    keywords of replay_move.  Every move n - 1 -> n is replayed in longdouble (the reference) and in float64 from
    states[n - 1], and for every (walker, move) that is fragile in neither:
      * the end row is the reference's within tol_u * scale (circular_distance; scale: the reference's, see Conditioning);
      * a walker the reference leaves in place is bit for bit its previous state;
    for every move none of whose walkers is fragile, ncalls[n] - ncalls[n - 1] is the reference's calls, exactly (per group);
    theta and logl are, bit for bit, evaluate(u) for every row of every prefix; ncalls never decreases.  At most FRAGILE_CAP
    of the pairs may be fragile or loose (tol_u * scale above TOL_CEILING: no end-row comparison) and at least one move must be
    compared with exact calls.  Returns the figures: pairs, fragile, loose, exact_moves, worst (largest end-row error / scale),
    worst_abs (largest end-row error as it is), max_scale (largest scale compared), spread (largest float64 - longdouble
    distance / scale)."""
    N = len(states) - 1
    K = states[0][0].shape[0]
    groups = np.zeros(K, dtype=np.intp) if groups is None else np.asarray(groups, dtype=np.intp)
    ngroups = int(groups.max()) + 1 if K else 1
    calls = np.asarray(ncalls, dtype=np.int64).reshape(N + 1, -1)
    assert calls.shape[1] == ngroups and np.all(calls[0] == 0) and np.all(np.diff(calls, axis=0) >= 0)
    left = np.full(K, N) if steps is None else np.asarray(steps)[groups]
    fig = SimpleNamespace(pairs=0, fragile=0, loose=0, exact_moves=0, worst=0.0, worst_abs=0.0, max_scale=1.0, spread=0.0)
    for n in range(N + 1):
        th, ll = evaluate(np.ascontiguousarray(states[n][0]))
        assert np.array_equal(np.asarray(th).reshape(K, -1), states[n][1]) and np.array_equal(ll, states[n][2]), n
    for n in range(1, N + 1):
        (u0, t0, l0), (u1, t1, l1) = states[n - 1], states[n]
        on = left >= n                                              # walkers that make move n - 1
        same = np.all(u1 == u0, axis=1) & np.all(t1 == t0, axis=1) & (l1 == l0)
        assert same[~on].all(), ("a walker past its run's moves changed", n)
        if not on.any():
            continue
        sub = {k: (np.asarray(v)[on] if k in ("seed", "wid", "lstar") and np.ndim(v) == 1 else
                   np.asarray(v)[on] if k == "chol" and np.ndim(v) == 3 else v) for k, v in walk.items()}
        ref = replay_move(u0[on], t0[on], l0[on], n - 1, wrapped=wrapped, evaluate=evaluate, dtype=np.longdouble, **sub)
        f64 = replay_move(u0[on], t0[on], l0[on], n - 1, wrapped=wrapped, evaluate=evaluate, dtype=np.float64, **sub)
        good = ~(ref.fragile | f64.fragile)
        fig.pairs += int(on.sum())
        fig.fragile += int((~good).sum())
        assert np.array_equal(ref.moved[good], f64.moved[good]) and np.array_equal(ref.calls[good], f64.calls[good]), n
        tight = good & (tol_u * ref.scale <= TOL_CEILING)           # the pairs whose end rows are compared
        fig.loose += int((good & ~tight).sum())
        if tight.any():
            fig.spread = max(fig.spread, float((circular_distance(f64.u, ref.u, wrapped) / ref.scale)[tight].max()))
        err = circular_distance(u1[on].astype(np.longdouble), ref.u, wrapped) / ref.scale
        bad = np.flatnonzero(tight & ~(err <= tol_u))
        assert bad.size == 0, _explain(n, np.flatnonzero(on)[bad[0]], bad.size, err[bad[0]], ref, bad[0], u0[on], u1[on])
        if tight.any():
            fig.worst = max(fig.worst, float(err[tight].max()))
            fig.worst_abs = max(fig.worst_abs, float((err * ref.scale)[tight].max()))
            fig.max_scale = max(fig.max_scale, float(ref.scale[tight].max()))
        stay = good & ~ref.moved
        assert same[on][stay].all(), ("the reference gives the move up, the walk moved", n, np.flatnonzero(on)[stay & ~same[on]][:5])
        for g in range(ngroups):
            mine = groups[on] == g
            if mine.any() and good[mine].all():
                assert calls[n, g] - calls[n - 1, g] == int(ref.calls[mine].sum()), \
                    ("calls of a move", n, g, int(calls[n, g] - calls[n - 1, g]), int(ref.calls[mine].sum()))
                fig.exact_moves += 1
    assert fig.fragile + fig.loose <= FRAGILE_CAP * fig.pairs, ("too many fragile or loose pairs", fig.fragile, fig.loose, fig.pairs)
    assert fig.exact_moves >= 1
    return fig


def _explain(n, walker, nbad, err, ref, i, u0, u1):
    return (f"move {n - 1}: {nbad} walkers off the reference; walker {walker}: error / scale {float(err):.3e}, scale {float(ref.scale[i]):.1f}, start {u0[i]}, "
            f"end {u1[i]}, reference end {ref.u[i].astype(np.float64)}, d {ref.d[i].astype(np.float64)}, "
            f"bracket [{float(ref.lo[i])}, {float(ref.hi[i])}], calls {int(ref.calls[i])}, moved {bool(ref.moved[i])}")
