"""CPU: nested.run_nested_ensemble(live=...) — the live sets of R runs resident side by side, sorted, whitened and walked
together (GpuRVModel.live_runs_*) — is R runs of run_nested_slice(live=...) with the order on the "device", bit for bit, when
both are fed the same deterministic host walk; and the evidence sums vectorised across runs are the one-run sums row by row."""
import numpy as np
import pytest

from evidence_amd import run_nested_ensemble
from evidence_amd.nested import _deaths, _deaths_runs, run_nested_slice


def prior(cube):
    return -10.0 + 20.0 * cube                                      # Uniform(-10, 10)


def loglike(x):
    return -0.5 * np.sum(x * x, axis=1)


def walk(cube, theta, logl, lstar, chol, wrapped, nsteps, max_rounds, seed):
    """A crude but deterministic constrained move whose call count depends on the seed (rejections cost extra)."""
    rng = np.random.default_rng(seed)
    c = cube.copy()
    used = 0
    for _ in range(nsteps):
        prop = np.clip(c + (rng.standard_normal(c.shape) @ chol.T) * 0.5, 0.0, np.nextafter(1.0, 0.0))
        ok = loglike(prior(prop)) > lstar
        used += len(c) + int(np.sum(~ok))
        c[ok] = prop[ok]
    th = prior(c)
    return c, th, loglike(th), used


class _OneRun:
    """A numpy stand-in for one model's resident live set with the order on the "device" (live_init / live_sort / live_step
    with ranks / live_get / live_dead), as tests/test_nested_host.py has it."""

    def live_init(self, cube):
        self.u = np.array(cube)
        self.theta = prior(self.u)
        self.logl = loglike(self.theta)
        self.dead_theta, self.dead_logl = [], []
        self.sorted_for = None
        return self.logl.copy()

    def live_sort(self, kdead):
        self.order = np.argsort(self.logl, kind="stable")
        self.sorted_for = kdead
        dl = self.logl[self.order[:kdead]]
        return dl.copy(), float(dl[-1]), float(self.logl[self.order[-1]])

    def live_step(self, order, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seed=0):
        assert order is None and self.sorted_for == kdead and lstar == self.logl[self.order[kdead - 1]]
        self.sorted_for = None
        ranks = np.asarray(ranks)
        assert ranks.shape == (kdead,) and ranks.min() >= 0 and ranks.max() < len(self.logl) - kdead
        dead, alive = self.order[:kdead], self.order[kdead:]
        start = alive[ranks]
        self.dead_theta.append(self.theta[dead].copy()); self.dead_logl.append(self.logl[dead].copy())
        ua = self.u[alive]
        d0 = ua - ua.mean(axis=0)
        chol = np.linalg.cholesky(d0.T @ d0 / max(1, len(alive) - 1) + 1e-14 * np.eye(self.u.shape[1]))
        wu, wt, wl, used = walk(self.u[start], self.theta[start], self.logl[start], lstar, chol, wrapped, nsteps, max_rounds, seed)
        self.u[dead], self.theta[dead], self.logl[dead] = wu, wt, wl
        return wl.copy(), used

    def live_get(self, cube=True, theta=True, logl=True):
        return (self.u.copy() if cube else None, self.theta.copy() if theta else None, self.logl.copy() if logl else None)

    def live_dead(self):
        return np.vstack(self.dead_theta), np.concatenate(self.dead_logl)


class _Runs:
    """A numpy stand-in for GpuRVModel.live_runs_*: R one-run live sets behind the ensemble interface, with its call rules
    (step after a sort of the same runs and kdead, the lstar it returned, runs distinct and ascending).  Records the runs of
    every step."""

    def __init__(self):
        self.steps = []

    def live_runs_init(self, cube, nruns):
        n = len(cube) // nruns
        assert n * nruns == len(cube)
        self.runs = [_OneRun() for _ in range(nruns)]
        return np.stack([r.live_init(cube[i * n:(i + 1) * n]) for i, r in enumerate(self.runs)])

    def live_runs_sort(self, runs, kdead):
        runs = [int(r) for r in runs]
        assert runs == sorted(set(runs)) and runs[-1] < len(self.runs)
        got = [self.runs[r].live_sort(kdead) for r in runs]
        self.sorted = (runs, kdead, [g[1] for g in got])
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got]), np.array([g[2] for g in got])

    def live_runs_step(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=()):
        runs = [int(r) for r in runs]
        assert self.sorted == (runs, kdead, [float(v) for v in lstar])
        self.sorted = None
        assert np.shape(ranks) == (len(runs), kdead) and len(seeds) == len(runs)
        self.steps.append(runs)
        got = [self.runs[r].live_step(None, kdead, ranks[j], lstar[j], wrapped, nsteps, max_rounds, seeds[j])
               for j, r in enumerate(runs)]
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64)

    def live_runs_get(self, run, cube=True, theta=True, logl=True, theta_out=None):
        u, th, ll = self.runs[run].live_get(cube, theta or theta_out is not None, logl)
        if theta_out is not None:
            theta_out[...] = th
        return u, th, ll

    def live_runs_dead_count(self, run):
        return sum(len(a) for a in self.runs[run].dead_logl)

    def live_runs_dead(self, run, theta_out=None):
        th, ll = self.runs[run].live_dead()
        if theta_out is not None:
            theta_out[...] = th
        return th, ll


KW = dict(nlive=120, kbatch=10, nsteps=3, dlogz=0.1, max_calls=400_000)


def _same(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall
    assert a.logz == b.logz and a.logzerr == b.logzerr and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)


def _alone(ndim, seed, kw):
    return run_nested_slice(None, None, ndim, seed=seed, live=_OneRun(), **kw)


def _check_lockstep(live, got, kbatch):
    # one step per lockstep iteration, holding exactly the runs that had not stopped
    turns = [g.niter // kbatch for g in got]
    assert len(live.steps) == max(turns)
    assert [len(s) for s in live.steps] == [sum(t > i for t in turns) for i in range(max(turns))]
    assert all(g.timing["turns"] == t for g, t in zip(got, turns))


@pytest.mark.parametrize("seeds", [(5,), (1, 2, 3), (11, 12, 13, 14, 15, 16, 17)])
def test_resident_ensemble_is_the_standalone_resident_runs(seeds):
    live = _Runs()
    got = run_nested_ensemble(None, None, 3, seeds, live=live, **KW)
    assert len(got) == len(seeds)
    for s, g in zip(seeds, got):
        _same(g, _alone(3, s, KW))
    _check_lockstep(live, got, KW["kbatch"])


@pytest.mark.parametrize("nseeds", [3, 7])
def test_runs_that_stop_at_different_iterations(nseeds):
    seeds = list(range(40, 40 + nseeds))
    kw = dict(KW, dlogz=0.5, kbatch=5)
    live = _Runs()
    got = run_nested_ensemble(None, None, 2, seeds, live=live, **kw)
    assert len({g.niter for g in got}) > 1
    for s, g in zip(seeds, got):
        _same(g, _alone(2, s, kw))
    _check_lockstep(live, got, kw["kbatch"])


@pytest.mark.parametrize("seeds", [(1,), (21, 22, 23), (31, 32, 33, 34, 35, 36, 37)])
def test_one_run_hits_max_calls(seeds):
    free = [_alone(3, s, KW) for s in seeds]
    ncalls = sorted(f.ncall for f in free)
    budget = ncalls[-2] + 1 if len(seeds) > 1 else ncalls[-1] // 2
    kw = dict(KW, max_calls=budget)
    live = _Runs()
    got = run_nested_ensemble(None, None, 3, seeds, live=live, **kw)
    cut = [g for g, f in zip(got, free) if g.niter < f.niter]
    assert len(cut) == 1 and cut[0].ncall >= budget
    for s, g in zip(seeds, got):
        _same(g, _alone(3, s, kw))
    _check_lockstep(live, got, KW["kbatch"])


def test_max_iter_cuts_every_run():
    seeds = (3, 4, 5)
    kw = dict(KW, max_iter=35)                       # not a multiple of kbatch: the last turn overshoots, as a standalone run's
    live = _Runs()
    got = run_nested_ensemble(None, None, 3, seeds, live=live, **kw)
    assert all(g.niter == 40 for g in got)
    for s, g in zip(seeds, got):
        _same(g, _alone(3, s, kw))


@pytest.mark.parametrize("kbatch", [1, 7, 100, 300])
def test_deaths_over_runs_is_deaths_row_by_row(kbatch):
    rng = np.random.default_rng(kbatch)
    nlive, A = 400, 9
    logx = -float(rng.uniform(0.0, 30.0))
    dl = np.sort(rng.normal(-50.0, 20.0, (A, kbatch)), axis=1)
    dl[1] = dl[1, 0]                                          # ties
    dl[2, : kbatch // 2] = -1e30                              # the invalid-orbit log-L
    logz = rng.normal(-60.0, 20.0, A)
    logz[0] = -np.inf                                         # the first iteration
    logz[3] = dl[3, -1] + 40.0                                # logz far above the shells
    h = rng.uniform(0.0, 10.0, A)
    h[0] = 0.0
    logw, lz, hh, lx = _deaths_runs(logz, h, logx, dl, nlive, kbatch)
    for a in range(A):
        w1, z1, h1, x1 = _deaths(float(logz[a]), float(h[a]), logx, dl[a], nlive, kbatch)
        assert np.array_equal(logw[a], w1) and lz[a] == z1 and hh[a] == h1 and lx == x1, a
        assert np.array_equal(np.signbit(logw[a]), np.signbit(w1))
    # chained over iterations, as the ensemble uses it: every run stays on its own one-run sums
    one = [(-np.inf, 0.0, 0.0)] * A
    lz, hh, lx = np.full(A, -np.inf), np.zeros(A), 0.0
    for it in range(5):
        dl = np.sort(rng.normal(-40.0 + 5 * it, 10.0, (A, kbatch)), axis=1)
        _, lz, hh, lx = _deaths_runs(lz, hh, lx, dl, nlive - 0, kbatch)
        one = [_deaths(z, hv, x, dl[a], nlive, kbatch)[1:] for a, (z, hv, x) in enumerate(one)]
        assert all(lz[a] == z and hh[a] == hv and lx == x for a, (z, hv, x) in enumerate(one))


def test_argument_errors():
    with pytest.raises(ValueError):
        run_nested_ensemble(None, None, 2, (1, 2), live=_Runs(), clustering=True, **KW)
    with pytest.raises(ValueError):
        run_nested_ensemble(None, None, 2, (1, 2), live=_Runs(), walker_runs=lambda *a: None, **KW)
    with pytest.raises(ValueError):
        run_nested_ensemble(None, None, 2, [], live=_Runs(), **KW)
    with pytest.raises(ValueError):
        run_nested_ensemble(None, None, 2, (1, 2), live=_Runs(), **dict(KW, kbatch=KW["nlive"]))
