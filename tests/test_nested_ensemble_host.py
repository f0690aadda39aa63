"""CPU: nested.run_nested_ensemble — R independent runs in lockstep, their walks in one call per iteration — is R runs of
run_nested_slice(walker=...), bit for bit, when both are fed the same deterministic host walk."""
import numpy as np
import pytest

from evidence_amd import run_nested_ensemble
from evidence_amd.nested import run_nested_slice


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


class _WalkerRuns:
    """walker_runs for run_nested_ensemble: `walk` applied run by run; records the runs of every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
        R = len(run_start) - 1
        assert len(lstar) == R and chol.shape[0] == R and len(seeds) == R and run_start[-1] == len(cube)
        self.calls.append((R, [float(v) for v in lstar]))
        cube, theta, logl = cube.copy(), theta.copy(), logl.copy()
        ncalls = np.zeros(R, dtype=np.int64)
        for r in range(R):
            rows = slice(run_start[r], run_start[r + 1])
            cube[rows], theta[rows], logl[rows], ncalls[r] = walk(cube[rows], theta[rows], logl[rows], lstar[r], chol[r],
                                                                  wrapped, nsteps, max_rounds, seeds[r])
        return cube, theta, logl, ncalls


KW = dict(nlive=120, kbatch=10, nsteps=3, dlogz=0.1, max_calls=400_000)


def _same(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall
    assert a.logz == b.logz and a.logzerr == b.logzerr and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)


def _check_lockstep(wr, got, kbatch):
    # one call per lockstep iteration, holding exactly the runs that had not stopped
    turns = [r.niter // kbatch for r in got]
    assert len(wr.calls) == max(turns)
    assert [n for n, _ in wr.calls] == [sum(t > i for t in turns) for i in range(max(turns))]


@pytest.mark.parametrize("seeds", [(5,), (1, 2, 3), (11, 12, 13, 14, 15, 16, 17)])
def test_ensemble_is_the_standalone_runs_gaussian(seeds):
    wr = _WalkerRuns()
    got = run_nested_ensemble(prior, loglike, 3, seeds, walker_runs=wr, **KW)
    assert len(got) == len(seeds)
    for s, g in zip(seeds, got):
        _same(g, run_nested_slice(prior, loglike, 3, seed=s, walker=walk, **KW))
    _check_lockstep(wr, got, KW["kbatch"])


@pytest.mark.parametrize("nseeds", [3, 7])
def test_runs_that_stop_at_different_iterations(nseeds):
    # a 2-D problem with a coarse stop: the runs end at different iterations and leave the lockstep one by one
    seeds = list(range(40, 40 + nseeds))
    kw = dict(KW, dlogz=0.5, kbatch=5)
    wr = _WalkerRuns()
    got = run_nested_ensemble(prior, loglike, 2, seeds, walker_runs=wr, **kw)
    assert len({g.niter for g in got}) > 1
    for s, g in zip(seeds, got):
        _same(g, run_nested_slice(prior, loglike, 2, seed=s, walker=walk, **kw))
    _check_lockstep(wr, got, kw["kbatch"])
    # a run that has stopped is never walked again: the lstar it would get next is not in the later calls
    assert all(len(lst) == n for n, lst in wr.calls)


@pytest.mark.parametrize("seeds", [(1,), (21, 22, 23), (31, 32, 33, 34, 35, 36, 37)])
def test_one_run_hits_max_calls(seeds):
    free = [run_nested_slice(prior, loglike, 3, seed=s, walker=walk, **KW) for s in seeds]
    ncalls = sorted(f.ncall for f in free)
    # a budget that only the most expensive run reaches (the one run, for a single seed)
    budget = ncalls[-2] + 1 if len(seeds) > 1 else ncalls[-1] // 2
    kw = dict(KW, max_calls=budget)
    wr = _WalkerRuns()
    got = run_nested_ensemble(prior, loglike, 3, seeds, walker_runs=wr, **kw)
    cut = [g for g, f in zip(got, free) if g.niter < f.niter]
    assert len(cut) == 1 and cut[0].ncall >= budget
    for s, g in zip(seeds, got):
        _same(g, run_nested_slice(prior, loglike, 3, seed=s, walker=walk, **kw))
    _check_lockstep(wr, got, KW["kbatch"])


def test_initial_live_points_are_one_callback_call():
    seen = []

    def counting_prior(c):
        seen.append(c.shape)
        return prior(c)

    run_nested_ensemble(counting_prior, loglike, 2, (1, 2, 3), walker_runs=_WalkerRuns(), **dict(KW, max_calls=1000))
    assert seen == [(3 * KW["nlive"], 2)]


def test_argument_errors():
    with pytest.raises(ValueError):
        run_nested_ensemble(prior, loglike, 2, [], walker_runs=_WalkerRuns(), **KW)
    with pytest.raises(ValueError):
        run_nested_ensemble(prior, loglike, 2, (1, 2), walker_runs=_WalkerRuns(), **dict(KW, kbatch=KW["nlive"]))
    with pytest.raises(ValueError):
        run_nested_ensemble(prior, loglike, 2, (1, 2), **KW)
