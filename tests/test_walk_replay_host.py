"""CPU: the replay of the device walk's moves (tests/walk_replay.py) is itself checked — its counters are disjoint for every
argument the entry accepts, its moves keep the walk's invariants on an analytic likelihood, they are the host walks' moves
(stepout.walk fed the counter draws: the same candidates; both host walks with a numpy generator: the same distribution), and
the float64 and longdouble replays decide every move alike that is not fragile, with the fragile share under the cap for the
shapes test_gpu_walk_replay.py runs."""
import numpy as np
import pytest
from scipy import stats

import walk_replay as wr
from evidence_amd import stepout
from evidence_amd.callbacks import wrapped_params
from evidence_amd.layout import compile_layout
from evidence_amd.nested import _chord
from evidence_amd.synthetic import make_workload

from walk_replay import SPREAD, TOL_U


def gaussian(mu, sig, wrapped):
    """An off-centre Gaussian in the cube; periodic (through sin) in the wrapped coordinates.  theta = the cube row."""
    mu, sig, wrapped = np.asarray(mu), np.asarray(sig), np.asarray(wrapped, dtype=bool)

    def evaluate(c):
        z = np.where(wrapped, np.sin(np.pi * (c - mu)) / np.pi, c - mu) / sig
        return c.copy(), -0.5 * np.sum(z * z, axis=1)
    return evaluate


def oracle_evaluate(cfg):
    """prior transform + log-L of a synthetic configuration by the CPU oracles (priors_oracle.ppf, the C log-L)."""
    from oracle import priors_oracle as po
    from oracle.oracle import OracleModel
    w = make_workload(cfg)
    layout = compile_layout(w.parnames, w.fixedpardict, list(w.table.insts))
    om = OracleModel(layout, w.table)
    pri = [w.input_dict[n.rsplit("_", 1)[0]][n.rsplit("_", 1)[1]][2] for n in layout.parnames]

    def evaluate(c):
        theta = np.ascontiguousarray(np.stack([po.ppf(p[0], p[1:], c[:, j]) for j, p in enumerate(pri)], axis=1))
        return theta, om.loglike(theta, nthreads=8)
    return evaluate, wrapped_params(list(layout.parnames))


def start(evaluate, ndim, k, seed, quantile):
    """As _start of test_gpu_walk.py: uniform rows above the quantile's log-L, and their covariance's factor."""
    rng = np.random.default_rng(seed)
    cube = rng.random((k, ndim))
    theta, logl = evaluate(cube)
    lstar = -np.inf if quantile is None else float(np.quantile(logl, quantile))
    keep = logl > lstar
    cube, theta, logl = cube[keep], theta[keep], logl[keep]
    d0 = cube - cube.mean(axis=0)
    chol = np.linalg.cholesky(d0.T @ d0 / (len(cube) - 1) + 1e-14 * np.eye(ndim))
    return cube, theta, logl, lstar, chol


D4 = dict(mu=[0.3, 0.62, 0.9, 0.45], sig=[0.08, 0.2, 0.15, 0.3], wrapped=[False, True, True, False])


def test_counter_ranges_are_disjoint_for_every_accepted_argument():
    # the three fields never run into each other: draw < 2^14, move < 2^18 (<< 14: below bit 32), walker id < 2^32
    top_normal = lambda D: 2 * ((D - 1) * D + (D - 1)) + 1               # the second uniform of the last basis normal
    assert all(top_normal(D) < wr.SHRINK_DRAW for D in range(1, wr.STEPOUT_MAX_NDIM + 1))
    assert top_normal(wr.STEPOUT_MAX_NDIM) == wr.SHRINK_DRAW - 1         # 64 parameters use the range up, exactly ...
    assert top_normal(wr.STEPOUT_MAX_NDIM + 1) >= wr.SHRINK_DRAW         # ... and 65 would reach the shrink draws: refused
    with pytest.raises(ValueError):
        wr.replay_move(np.full((1, 65), 0.5), np.zeros((1, 65)), np.zeros(1), 0, proposal="stepout", seed=1, wid=0, lstar=-1.0,
                       chol=np.eye(65), wrapped=None, max_rounds=5, evaluate=None)
    assert wr.SHRINK_DRAW + wr.MAX_ROUNDS - 1 < wr.OFFSET_DRAW < 1 << 14
    assert (wr.MAX_NSTEPS - 1) << 14 | ((1 << 14) - 1) < 1 << 32
    big = int(wr.counter(2 ** 32 - 1, wr.MAX_NSTEPS - 1, wr.OFFSET_DRAW))
    assert big == ((2 ** 32 - 1) << 32) | ((wr.MAX_NSTEPS - 1) << 14) | wr.OFFSET_DRAW and big < 2 ** 64
    # (a chord walk's 2 D normal draws stay below the shrink draws up to 4096 parameters — far more than a workgroup holds)
    # and written out for a small walk: every counter a walk of 3 walkers, 7 moves, 5 rounds touches is its own
    for proposal, D in (("chord", 3), ("stepout", 3), ("stepout", 64)):
        seen = []
        for wid in (0, 1, 2 ** 32 - 1):
            for m in range(7):
                if proposal == "chord":
                    seen += [int(wr.counter(wid, m, 2 * k + h)) for k in range(D) for h in (0, 1)]
                else:
                    if m % D == 0 or m == 0:
                        seen += [int(wr.counter(wid, m // D, 2 * (v * D + k) + h)) for v in range(D) for k in range(D) for h in (0, 1)]
                    seen.append(int(wr.counter(wid, m, wr.OFFSET_DRAW)))
                seen += [int(wr.counter(wid, m, wr.SHRINK_DRAW + r)) for r in range(5)]
        assert len(set(seen)) == len(seen), (proposal, D)


def test_uniform_and_normal_are_the_documented_draws():
    from evidence_amd.shrinkage import uniform01
    ctr = wr.counter(5, 3, np.arange(0, 40, 2))
    assert ctr[1] == (5 << 32) | (3 << 14) | 2
    assert np.array_equal(wr.uniform(9, np.arange(50, dtype=np.uint64)), uniform01(np.array([9], dtype=np.uint64), 50)[0])
    z = wr.normal(9, ctr)
    u1, u2 = wr.uniform(9, ctr), wr.uniform(9, ctr + np.uint64(1))
    assert z.dtype == np.longdouble
    assert np.allclose(z.astype(float), np.sqrt(-2 * np.log(1 - u1)) * np.cos(2 * np.pi * u2), rtol=1e-14, atol=1e-15)
    many = wr.normal(3, np.arange(0, 400000, 2, dtype=np.uint64), np.float64)
    assert stats.kstest(many, "norm").pvalue > 1e-3
    g = np.random.default_rng(2).standard_normal((40, 6, 6))
    assert np.array_equal(wr.gram_schmidt(g), stepout.gram_schmidt(g))          # the host definition, bit for bit in float64
    g = np.random.default_rng(3).standard_normal((40, 19, 19))
    assert np.abs(wr.gram_schmidt(g) - stepout.gram_schmidt(g)).max() < 1e-12     # (numpy sums 19 terms pairwise)
    assert np.abs(wr.gram_schmidt(g.astype(np.longdouble), 5).astype(float) - stepout.gram_schmidt(g)[:, :5]).max() < 1e-12


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_moves_keep_the_walks_invariants(proposal):
    ev = gaussian(**D4)
    wrapped = np.array(D4["wrapped"])
    cube, theta, logl, lstar, chol = start(ev, 4, 1200, 1, 0.7)
    kw = dict(proposal=proposal, seed=11, wid=np.arange(len(cube)), chol=chol, wrapped=wrapped, evaluate=ev, step_width=1.0)
    states, ncalls, _ = wr.walk(cube, theta, logl, 9, lstar=lstar, max_rounds=200, **kw)
    for u, t, l in states:
        assert (l > lstar).all() and ((u >= 0) & (u < 1)).all() and np.array_equal(ev(u)[1], l)
    assert np.mean(np.any(states[-1][0] != cube, axis=1)) > 0.99 and ncalls[-1] > 9 * len(cube)
    # no constraint: the first shrink candidate of every move is accepted (chord: one call a move; stepout: the ends it
    # evaluates on the way out, each one width further, and then the one)
    free, nfree, _ = wr.walk(cube, theta, logl, 5, lstar=-np.inf, max_rounds=200, **kw)
    assert all(np.all(np.any(a[0] != b[0], axis=1)) for a, b in zip(free, free[1:]))
    if proposal == "chord":
        assert nfree == [m * len(cube) for m in range(6)]
    else:
        r = wr.replay_move(*free[0], 0, lstar=-np.inf, max_rounds=200, **kw)
        v = wr.uniform(11, wr.counter(np.arange(len(cube)), 0, wr.OFFSET_DRAW))
        cmin, cmax = stepout.wall_chord(cube, r.d.astype(float), wrapped)
        right = np.where(1 - v < cmax, np.ceil(cmax - (1 - v)), 0)                          # ends evaluated: hi0, hi0 + 1, .. < cmax
        left = np.where(-v > cmin, np.ceil(-v - cmin), 0)
        assert np.array_equal(r.calls, (right + left + 1).astype(np.int64))
        assert np.allclose(r.lo.astype(float), cmin, rtol=1e-12) and np.allclose(r.hi.astype(float), cmax, rtol=1e-12)   # out to the walls
    # max_rounds = 1 .. 3: a move that runs out of rounds leaves the walker where it is, and costs exactly max_rounds calls
    tight = start(ev, 4, 6000, 2, 0.97)
    for mr in (1, 2, 3):
        r = wr.replay_move(*tight[:3], 0, lstar=tight[3], max_rounds=mr, **dict(kw, wid=np.arange(len(tight[0])), chol=tight[4]))
        stay = ~r.moved
        assert stay.any() and np.all(r.calls[stay] == mr) and np.all(r.calls <= mr)
        # (a stepout move spends its first rounds on the two ends of its bracket: with one or two it moves only if the walls cut them)
        assert r.moved.any() or (proposal == "stepout" and mr < 3)
        assert np.array_equal(r.u[stay].astype(float), tight[0][stay]) and np.array_equal(r.logl[stay], tight[2][stay])
        assert (r.logl > tight[3]).all()


def test_a_zero_row_of_the_factor_sets_no_limit():
    ev = gaussian(**D4)
    cube, theta, logl, lstar, chol = start(ev, 4, 400, 3, 0.5)
    flat = chol.copy()
    flat[2, :] = 0.0                                            # d_2 == 0 exactly: (0 - u) / 0 must not reach the chord
    for proposal in ("chord", "stepout"):
        r = wr.replay_move(cube, theta, logl, 1, proposal=proposal, seed=4, wid=np.arange(len(cube)), lstar=lstar, chol=flat,
                           wrapped=np.zeros(4, dtype=bool), max_rounds=200, evaluate=ev)
        assert np.all(r.d[:, 2] == 0) and np.isfinite(r.lo).all() and np.isfinite(r.hi).all() and (r.lo < 0).all() and (r.hi > 0).all()
        assert np.array_equal(r.u[:, 2].astype(float), cube[:, 2]) and r.moved.mean() > 0.9 and (r.logl > lstar).all()
        lo, hi = (_chord if proposal == "chord" else stepout.wall_chord)(cube, r.d.astype(float), np.zeros(4, dtype=bool))
        assert np.isfinite(lo).all() and np.isfinite(hi).all()


class CounterRng:
    """The draws stepout.walk asks a numpy generator for, answered from the device's counters for ONE walker: the normals of
    basis b when a move m = b D begins, the offset of the move as its first uniform, then the shrink uniform of the round the
    move is in.  evaluated() is told every log-L the walk computes, which is how the rounds and the end of a move are known."""

    def __init__(self, seed, wid, ndim, max_rounds, lstar):
        self.seed, self.wid, self.D, self.max_rounds, self.lstar = seed, wid, ndim, max_rounds, lstar
        self.m, self.new, self.round, self.pending = -1, True, 0, False

    def standard_normal(self, shape):
        D = self.D
        assert self.new and (self.m + 1) % D == 0
        draws = 2 * (np.arange(D)[:, None] * D + np.arange(D)[None, :])
        return wr.normal(self.seed, wr.counter(self.wid, (self.m + 1) // D, draws), np.float64).reshape(shape)

    def random(self, n):
        assert n == 1
        if self.new:
            self.m, self.new, self.round, self.pending = self.m + 1, False, 0, False
            return wr.uniform(self.seed, wr.counter(self.wid, self.m, wr.OFFSET_DRAW)).reshape(1)
        self.pending = True
        return wr.uniform(self.seed, wr.counter(self.wid, self.m, wr.SHRINK_DRAW + self.round)).reshape(1)

    def evaluated(self, ll):
        self.round += 1
        if (self.pending and ll > self.lstar) or self.round >= self.max_rounds:
            self.new = True
        self.pending = False


@pytest.mark.parametrize("max_rounds, width", [(200, 0.7), (4, 0.3), (7, 3.0)])
def test_stepout_moves_are_stepout_walks_moves_fed_the_counter_draws(max_rounds, width):
    """stepout.walk, one walker at a time, with a generator that hands it the counter draws, makes the replay's moves: the same
    calls and (to rounding: its factor product goes through BLAS) the same end points after every walk.  This ties the
    replay's phases, its clamps, its counters and its round counting to the host definition."""
    ev = gaussian(**D4)
    wrapped = np.array(D4["wrapped"])
    cube, theta, logl, lstar, chol = start(ev, 4, 400, 5, 0.8)
    nsteps, seed = 6, 21
    states, ncalls, fragile = wr.walk(cube, theta, logl, nsteps, proposal="stepout", seed=seed, wid=np.arange(len(cube)) + 17,
                                      lstar=lstar, chol=chol, wrapped=wrapped, max_rounds=max_rounds, evaluate=ev, step_width=width)
    total = 0
    for i in np.flatnonzero(~fragile.any(axis=0)):
        rng = CounterRng(seed, i + 17, 4, max_rounds, lstar)

        def evaluate(c):
            th, ll = ev(c)
            rng.evaluated(ll[0])
            return th, ll
        wu, wt, wl = cube[i:i + 1].copy(), theta[i:i + 1].copy(), logl[i:i + 1].copy()
        n = stepout.walk(wu, wt, wl, lstar, chol, wrapped, nsteps, max_rounds, width, rng, evaluate)
        assert np.abs(wu[0] - states[-1][0][i]).max() < 1e-13 and abs(wl[0] - states[-1][2][i]) < 1e-9, i
        total += n
    assert fragile.sum() <= 2
    if not fragile.any():
        assert total == ncalls[-1]


def _host_chord_walk(wu, wl, lstar, chol, wrapped, nsteps, rng, evaluate):
    """The chord walk of nested.run_nested_slice (its loop over nsteps, with one factor), drawing from a numpy generator."""
    k, ndim = wu.shape
    for _ in range(nsteps):
        z = rng.standard_normal((k, ndim))
        d = z @ chol.T
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        tmin, tmax = _chord(wu, d, wrapped)
        todo = np.arange(k)
        rounds = 0
        while todo.size and rounds < 200:
            t = tmin[todo] + (tmax[todo] - tmin[todo]) * rng.random(todo.size)
            cand = wu[todo] + t[:, None] * d[todo]
            cand[:, wrapped] %= 1.0
            cand = np.clip(cand, 0.0, np.nextafter(1.0, 0.0))
            ct, cl = evaluate(cand)
            ok = cl > lstar
            wu[todo[ok]], wl[todo[ok]] = cand[ok], cl[ok]
            rej = todo[~ok]
            neg = t[~ok] < 0
            tmin[rej[neg]] = t[~ok][neg]
            tmax[rej[~neg]] = t[~ok][~neg]
            todo = rej
            rounds += 1


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_replayed_moves_have_the_host_walks_distribution(proposal):
    """From one start set, the host walk (numpy generator) and the replay (counters) end in samples of the same distribution:
    a two-sample KS test per coordinate.  The one statistical statement here, and it is about the reference."""
    ev = gaussian(**D4)
    wrapped = np.array(D4["wrapped"])
    cube, theta, logl, lstar, chol = start(ev, 4, 10000, 8, 0.6)
    nsteps = 3
    states, _, _ = wr.walk(cube, theta, logl, nsteps, proposal=proposal, seed=77, wid=np.arange(len(cube)), lstar=lstar, chol=chol,
                           wrapped=wrapped, max_rounds=200, evaluate=ev, step_width=1.0)
    wu, wt, wl = cube.copy(), theta.copy(), logl.copy()
    rng = np.random.default_rng(5)
    if proposal == "stepout":
        stepout.walk(wu, wt, wl, lstar, chol, wrapped, nsteps, 200, 1.0, rng, ev)
    else:
        _host_chord_walk(wu, wl, lstar, chol, wrapped, nsteps, rng, ev)
    for j in range(4):
        assert stats.ks_2samp(states[-1][0][:, j], wu[:, j]).pvalue > 1e-3, j
        # (the moves are short of forgetting the start, so a walk that did not move at all would pass the test above)
        assert stats.ks_2samp(states[-1][0][:, j] - cube[:, j], wu[:, j] - cube[:, j]).pvalue > 1e-3, j


def _case(name):
    """The shapes of test_gpu_walk_replay.py with evaluators a CPU has: (evaluate, wrapped, start tuple, walk keywords, moves)."""
    if name.startswith("cfg"):
        cfg, k, q = {"cfg1": (1, 500, 0.5), "cfg1 high": (1, 1500, 0.9), "cfg3": (3, 300, 0.5), "cfg3 high": (3, 1200, 0.9)}[name]
        ev, wrapped = oracle_evaluate(cfg)
        ndim = len(wrapped)
        return ev, wrapped, start(ev, ndim, k, cfg, q), {}, (ndim + 2 if cfg == 1 else 4)
    ev, wrapped = gaussian(**D4), np.array(D4["wrapped"])
    st = start(ev, 4, 3000, 12, None if name == "free" else 0.5)
    cube, theta, logl, lstar, chol = st
    if name == "walls":
        cube = cube.copy()
        cube[0::4, 0], cube[1::4, 0], cube[2::4, 1], cube[3::4, 1] = 0.0, wr.ONE_BELOW, 0.0, wr.ONE_BELOW
        theta, logl = ev(cube)
        keep = logl > lstar
        st = (cube[keep], theta[keep], logl[keep], lstar, chol)
    kw = {"free": {}, "ordinary": {}, "walls": {}, "rounds 1": dict(max_rounds=1), "rounds 2": dict(max_rounds=2),
          "rounds 5": dict(max_rounds=5), "tiny factor": dict(chol=1e-6 * chol), "huge factor": dict(chol=50.0 * chol),
          "narrow": dict(step_width=0.05), "wide": dict(step_width=20.0),
          "high counters": dict(seed=2 ** 64 - 3, wid=np.arange(len(st[0])) + 2 ** 32 - len(st[0]) - 1),
          "zero row": dict(chol=chol * np.array([1.0, 1.0, 1.0, 0.0])[:, None]), "K 1": {}, "K 7": {}, "K 9": {},
          "live step": dict(wid=np.arange(50) + 1000, seed=99)}[name]
    if name in ("K 1", "K 7", "K 9", "live step"):
        k = 50 if name == "live step" else int(name[2:])
        st = (st[0][:k], st[1][:k], st[2][:k], lstar, chol)
    return ev, wrapped, st, kw, 10


CASES = ["cfg1", "cfg1 high", "cfg3", "cfg3 high", "free", "ordinary", "walls", "rounds 1", "rounds 2", "rounds 5", "tiny factor",
         "huge factor", "narrow", "wide", "high counters", "zero row", "K 1", "K 7", "K 9", "live step"]


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
@pytest.mark.parametrize("name", CASES)
def test_float64_and_longdouble_replays_agree_and_few_moves_are_fragile(name, proposal, capsys):
    """The float64 replay stands in for the device: check_prefixes — the comparison the GPU test makes — passes with the
    tolerance that test uses, the float64 - longdouble spread stays within the figure that tolerance was derived from, the
    fragile share is under the cap (none at all without a constraint), and at least one move is compared with exact calls."""
    ev, wrapped, (cube, theta, logl, lstar, chol), kw, nsteps = _case(name)
    walk = dict(dict(proposal=proposal, seed=31, wid=np.arange(len(cube)), lstar=lstar, chol=chol, max_rounds=200, step_width=1.0), **kw)
    states, ncalls, fragile = wr.walk(cube, theta, logl, nsteps, wrapped=wrapped, evaluate=ev, **walk)
    fig = wr.check_prefixes(states, ncalls, ev, tol_u=TOL_U, wrapped=wrapped, **walk)
    with capsys.disabled():
        print(f"\n{name:14s} {proposal:8s} pairs {fig.pairs:6d} fragile {fig.fragile:3d} loose {fig.loose:3d} exact moves "
              f"{fig.exact_moves:3d} spread/scale {fig.spread:.2e} max scale {fig.max_scale:8.1f} worst {fig.worst_abs:.2e}", end="")
    assert fig.spread <= SPREAD and fig.worst <= fig.spread and TOL_U < 1e-12
    assert fig.fragile + fig.loose <= wr.FRAGILE_CAP * fig.pairs and TOL_U * fig.max_scale <= wr.TOL_CEILING
    if proposal == "chord":
        assert fig.max_scale == 1.0 and fig.worst_abs <= TOL_U          # the half-turn limit: no coordinate goes further than one
    if name == "free":
        assert fig.fragile == 0 and fig.exact_moves == nsteps


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_run_mode_shape_with_per_run_arguments_and_steps(proposal):
    """check_prefixes' groups / steps branch (the run-mode GPU test's): four runs of unequal size with their own lstar, factor,
    seed and number of moves, the walker id its index inside its run, calls per run."""
    ev, wrapped = gaussian(**D4), np.array(D4["wrapped"])
    cube, theta, logl, lstar, chol = start(ev, 4, 1400, 21, 0.5)
    k = len(cube)
    sizes = np.array([5, k // 3, 130, k - 135 - k // 3])
    groups = np.repeat(np.arange(4), sizes)
    steps = np.array([8, 3, 5, 6])
    kw = dict(proposal=proposal, seed=np.array([3, 2 ** 64 - 1, 5, 2 ** 63], dtype=np.uint64)[groups], lstar=np.array([0.0, -1.0, -0.25, -3.0])[groups] + lstar,
              wid=np.concatenate([np.arange(n) for n in sizes]), chol=np.stack([chol, 0.5 * chol, 2.0 * chol, 0.1 * chol])[groups],
              max_rounds=200, step_width=0.8)
    states, calls = [(cube, theta, logl)], [np.zeros(4, dtype=np.int64)]
    for n in range(1, 9):
        on = steps[groups] >= n
        r = wr.replay_move(*[a[on] for a in states[-1]], n - 1, wrapped=wrapped, evaluate=ev, dtype=np.float64,
                           **{key: (v[on] if np.ndim(v) else v) for key, v in kw.items()})
        u, t, l = (a.copy() for a in states[-1])
        u[on], t[on], l[on] = r.u, r.theta, r.logl
        states.append((u, t, l))
        calls.append(calls[-1] + np.bincount(groups[on], weights=r.calls, minlength=4).astype(np.int64))
    fig = wr.check_prefixes(states, calls, ev, tol_u=TOL_U, wrapped=wrapped, groups=groups, steps=steps, **kw)
    assert fig.pairs == int(np.sum(sizes * steps)) and fig.exact_moves == int(steps.sum()) and fig.fragile == 0
    moved_late = states[8][0].copy()
    moved_late[groups == 1] = states[8][0][groups == 1][::-1]                  # run 1 (3 moves) changing at prefix 8: caught
    with pytest.raises(AssertionError):
        wr.check_prefixes(states[:8] + [(moved_late, ev(moved_late)[0], ev(moved_late)[1])], calls, ev, tol_u=TOL_U, wrapped=wrapped,
                          groups=groups, steps=steps, **kw)


def test_the_fragile_rule_flags_and_leaves_out_what_it_should():
    """No planned case meets a fragile pair (the margins are seven orders above rounding), so the rule is shown to work on a
    built one: lstar placed within eps_l of the log-L of a walker's first candidate."""
    ev, wrapped = gaussian(**D4), np.array(D4["wrapped"])
    cube, theta, logl, _, chol = start(ev, 4, 4000, 22, 0.5)
    k = len(cube)
    kw = dict(proposal="chord", seed=8, wid=np.arange(k), chol=chol, max_rounds=200)
    first = wr.replay_move(cube, theta, logl, 0, lstar=-np.inf, wrapped=wrapped, evaluate=ev, **kw).logl     # the first candidates' log-L
    base = float(first.min()) - 1.0
    near = np.zeros(k, dtype=bool)
    near[::500] = True                                                        # 4 of 2000 walkers: under the cap of 0.5 %
    lstar = np.where(near, first - 0.5e-9 * np.maximum(1.0, np.abs(first)), base)
    kw = dict(kw, lstar=lstar)
    r = wr.replay_move(cube, theta, logl, 0, wrapped=wrapped, evaluate=ev, **kw)
    assert near.sum() >= 2 and np.array_equal(r.fragile, near)
    far = wr.replay_move(cube, theta, logl, 0, wrapped=wrapped, evaluate=ev, **dict(kw, lstar=np.where(near, lstar - 1e-6, lstar)))
    assert not far.fragile.any()
    # a walk under test that decides the fragile pairs the other way (it stays, after 3 calls) passes; its move 0 is not
    # compared for calls, move 1 is; the same difference on a pair that is not fragile fails
    states, ncalls, _ = wr.walk(cube, theta, logl, 2, wrapped=wrapped, evaluate=ev, **kw)
    other = [states[0]] + [tuple(a.copy() for a in s) for s in states[1:]]
    for a, b in zip(other[1], states[0]):
        a[near] = b[near]
    second = wr.replay_move(*other[1], 1, wrapped=wrapped, evaluate=ev, dtype=np.float64, **kw)
    other[2] = (second.u, second.theta, second.logl)
    calls = [0, ncalls[1] + 2 * int(near.sum()), ncalls[1] + 2 * int(near.sum()) + int(second.calls.sum())]
    fig = wr.check_prefixes(other, calls, ev, tol_u=TOL_U, wrapped=wrapped, **kw)
    assert fig.fragile == int(near.sum()) and fig.exact_moves == 1
    with pytest.raises(AssertionError):
        wr.check_prefixes(other, calls, ev, tol_u=TOL_U, wrapped=wrapped, **dict(kw, lstar=np.where(near, lstar - 1e-6, lstar)))
    with pytest.raises(AssertionError):                                       # and the cap: every walker fragile
        wr.check_prefixes(states, ncalls, ev, tol_u=TOL_U, wrapped=wrapped, **dict(kw, eps_l=1e3))
