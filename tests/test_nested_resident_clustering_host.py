"""CPU: clustering inside the resident ensemble (run_nested_ensemble / run_nested_slice(live=..., clustering=True)).
A numpy stand-in of GpuRVModel.live_runs_* carries a live_runs_step_clustered written from the step's definition (global
whitening, metric scale, clustering.cluster_runs of the survivors in rank order, per-cluster factors, walker groups by the
cluster of their start row).  With the same deterministic walk, a resident clustered run is the host clustered run of its seed
bit for bit, an ensemble is its standalone runs, the bootstrap seeds are the host path's, and the new argument errors are
raised."""
import numpy as np
import pytest

from evidence_amd import run_nested_ensemble
from evidence_amd.clustering import cluster_runs
from evidence_amd.nested import (_BOOT_MUL, _M64, _cluster_factors, _cluster_scale, _covariance, _walk_groups,
                                 run_nested_slice)

SIG = 0.02
C1, C2 = np.full(3, 0.3), np.full(3, 0.7)
_CORR = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.9, 0.9, 1.0]])
_FLIP = np.diag([1.0, -1.0, 1.0])
COV1, COV2 = SIG ** 2 * _CORR, SIG ** 2 * _FLIP @ _CORR @ _FLIP


def _gauss_logpdf(x, c, cov):
    d = x - c
    sol = np.linalg.solve(cov, d.T).T
    return -0.5 * np.sum(d * sol, axis=1) - 0.5 * np.log(np.linalg.det(2 * np.pi * cov))


def mixture(x):
    return np.logaddexp(_gauss_logpdf(x, C1, COV1), _gauss_logpdf(x, C2, COV2)) + np.log(0.5)


def identity(cube):
    return np.array(cube, dtype=np.float64)


def box(cube):
    return -10.0 + 20.0 * cube


def gauss(x):
    return -0.5 * np.sum(x * x, axis=1)


class _Model:
    """prior, loglike and a crude but deterministic constrained walk whose calls depend on the seed, with the interfaces of
    GpuRVModel.slice_walk_runs (for the host path) and of one group of the stand-in's step."""

    def __init__(self, prior, loglike):
        self.prior, self.loglike = prior, loglike

    def walk(self, cube, lstar, chol, nsteps, seed):
        rng = np.random.default_rng(seed)
        c = cube.copy()
        used = 0
        for _ in range(nsteps):
            prop = np.clip(c + (rng.standard_normal(c.shape) @ chol.T) * 0.5, 0.0, np.nextafter(1.0, 0.0))
            ok = self.loglike(self.prior(prop)) > lstar
            used += len(c) + int(np.sum(~ok))
            c[ok] = prop[ok]
        th = self.prior(c)
        return c, th, self.loglike(th), used

    def walker_runs(self, cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
        out = [self.walk(cube[run_start[r]:run_start[r + 1]], lstar[r], chol[r], nsteps, seeds[r]) for r in range(len(seeds))]
        return (np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out]), np.concatenate([o[2] for o in out]),
                np.array([o[3] for o in out], dtype=np.int64))


class _OneRun:
    """One resident live set with the order on the "device"."""

    def __init__(self, model, cube):
        self.m = model
        self.u = np.array(cube)
        self.theta = model.prior(self.u)
        self.logl = model.loglike(self.theta)
        self.dead_theta, self.dead_logl = [], []

    def sort(self, kdead):
        self.order = np.argsort(self.logl, kind="stable")
        dl = self.logl[self.order[:kdead]]
        return dl.copy(), float(dl[-1]), float(self.logl[self.order[-1]])

    def step(self, kdead, ranks, lstar, wrapped, nsteps, seed, nboot=None, boot_seed=None):
        """The clustered step's definition (nboot given) or the unclustered one: (logl_new in walker order, calls, clusters)."""
        dead, alive = self.order[:kdead], self.order[kdead:]
        assert lstar == self.logl[dead[-1]]
        ranks = np.asarray(ranks)
        assert ranks.shape == (kdead,) and ranks.min() >= 0 and ranks.max() < len(alive)
        ua = self.u[alive]
        chol = np.linalg.cholesky(_covariance(ua))
        cw, factors, ncl = np.zeros(kdead, dtype=np.intp), [chol], 1
        if nboot is not None:
            labels, k, _ = cluster_runs(ua, [0, len(ua)], _cluster_scale(ua)[None, :], wrapped, nboot, [boot_seed])
            ncl = int(k[0])
            factors = _cluster_factors(ua, labels, ncl, chol)
            cw = labels.astype(np.intp)[ranks]
        wo, sizes, gf, gseeds = _walk_groups(cw, factors, seed)
        start = alive[ranks][wo]
        run_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        gu, gt, gl, used = self.m.walker_runs(self.u[start], self.theta[start], self.logl[start], run_start, [lstar] * len(sizes),
                                              np.stack(gf), wrapped, nsteps, 200, gseeds)
        self.dead_theta.append(self.theta[dead].copy()); self.dead_logl.append(self.logl[dead].copy())
        back = dead[wo]
        self.u[back], self.theta[back], self.logl[back] = gu, gt, gl
        wl = np.empty(kdead)
        wl[wo] = gl
        return wl, int(np.sum(used)), ncl


class _Runs:
    """A numpy stand-in for GpuRVModel.live_runs_*, with live_runs_step_clustered; records every step's runs and boot seeds."""

    def __init__(self, model):
        self.m = model
        self.steps = []

    def live_runs_init(self, cube, nruns):
        n = len(cube) // nruns
        self.runs = [_OneRun(self.m, cube[i * n:(i + 1) * n]) for i in range(nruns)]
        self.sorted = None
        return np.stack([r.logl.copy() for r in self.runs])

    def live_runs_sort(self, runs, kdead):
        runs = [int(r) for r in runs]
        assert runs == sorted(set(runs))
        got = [self.runs[r].sort(kdead) for r in runs]
        self.sorted = (runs, kdead, [g[1] for g in got])
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got]), np.array([g[2] for g in got])

    def _take(self, runs, kdead, lstar):
        runs = [int(r) for r in runs]
        assert self.sorted == (runs, kdead, [float(v) for v in lstar])
        self.sorted = None
        return runs

    def live_runs_step(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=()):
        runs = self._take(runs, kdead, lstar)
        self.steps.append((runs, None))
        got = [self.runs[r].step(kdead, ranks[j], lstar[j], wrapped, nsteps, seeds[j]) for j, r in enumerate(runs)]
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64)

    def live_runs_step_clustered(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=(), nboot=30,
                                 boot_seeds=()):
        runs = self._take(runs, kdead, lstar)
        assert len(seeds) == len(boot_seeds) == len(runs) and 0 <= nboot <= 32
        self.steps.append((runs, [int(b) for b in boot_seeds]))
        got = [self.runs[r].step(kdead, ranks[j], lstar[j], wrapped, nsteps, seeds[j], nboot, boot_seeds[j])
               for j, r in enumerate(runs)]
        return (np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64),
                np.array([g[2] for g in got], dtype=np.int32))

    def live_runs_get(self, run, cube=True, theta=True, logl=True, theta_out=None):
        r = self.runs[run]
        if theta_out is not None:
            theta_out[...] = r.theta
        return (r.u.copy() if cube else None, r.theta.copy() if theta else None, r.logl.copy() if logl else None)

    def live_runs_dead_count(self, run):
        return sum(len(a) for a in self.runs[run].dead_logl)

    def live_runs_dead(self, run, theta_out=None):
        th, ll = np.vstack(self.runs[run].dead_theta), np.concatenate(self.runs[run].dead_logl)
        if theta_out is not None:
            theta_out[...] = th
        return th, ll


KW = dict(nlive=150, kbatch=15, nsteps=3, dlogz=0.1, max_calls=400_000, nboot=16)
MIX = _Model(identity, mixture)


def _same(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall
    assert a.logz == b.logz and a.logzerr == b.logzerr and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)
    assert np.array_equal(a.nclusters, b.nclusters)


def _resident(seed, model=MIX, kw=KW):
    return run_nested_slice(None, None, 3, seed=seed, live=_Runs(model), clustering=True, **kw)


@pytest.mark.parametrize("seed", [3, 4])
def test_resident_clustered_run_is_the_host_clustered_run(seed):
    """Same draws, the same whitening, clusters, factors, groups and seeds: with the same walk the two paths give the same bits."""
    host = run_nested_slice(identity, mixture, 3, seed=seed, clustering=True, walker_runs=MIX.walker_runs, **KW)
    res = _resident(seed)
    _same(res, host)
    assert res.nclusters.max() >= 2 and res.nclusters.min() == 1           # both regimes are exercised
    assert set(res.timing) == {"host_s", "walk_s", "turns"}


@pytest.mark.parametrize("seeds", [(5,), (1, 2, 3), (11, 12, 13, 14, 15)])
def test_clustered_resident_ensemble_is_the_standalone_runs(seeds):
    live = _Runs(MIX)
    got = run_nested_ensemble(None, None, 3, seeds, live=live, clustering=True, **KW)
    assert len(got) == len(seeds)
    for s, g in zip(seeds, got):
        _same(g, _resident(s))
    turns = [g.niter // KW["kbatch"] for g in got]
    assert [len(r) for r, _b in live.steps] == [sum(t > i for t in turns) for i in range(max(turns))]
    assert all(b is not None for _r, b in live.steps)


def test_boot_seeds_are_the_host_paths():
    seeds = (7, 2 ** 63 + 5, 0)
    host_seen = []

    def recording(*args):
        host_seen.append(int(args[5][0]))
        return cluster_runs(*args)

    live = _Runs(MIX)
    run_nested_ensemble(None, None, 3, seeds, live=live, clustering=True, **KW)
    kb = KW["kbatch"]
    for j, s in enumerate(seeds):
        host_seen.clear()
        run_nested_slice(identity, mixture, 3, seed=s, clustering=True, clusterer=recording, walker_runs=MIX.walker_runs, **KW)
        mine = [b[r.index(j)] for r, b in live.steps if j in r]
        assert mine == host_seen
        # the deaths after the iteration's own: it = kbatch, 2 kbatch, ...
        assert mine == [(s * _BOOT_MUL + (t + 1) * kb) & _M64 for t in range(len(mine))]


def test_one_cluster_every_iteration_is_the_unclustered_resident_run():
    gm = _Model(box, gauss)
    kw = dict(KW, nlive=200, kbatch=20, dlogz=0.5)
    clustered = run_nested_slice(None, None, 3, seed=9, live=_Runs(gm), clustering=True, **kw)
    assert np.all(clustered.nclusters == 1)
    plain = run_nested_ensemble(None, None, 3, [9], live=_Runs(gm), **{k: v for k, v in kw.items() if k != "nboot"})[0]
    assert plain.nclusters is None
    for f in ("niter", "ncall", "logz", "logzerr", "information"):
        assert getattr(clustered, f) == getattr(plain, f)
    assert np.array_equal(clustered.samples, plain.samples) and np.array_equal(clustered.logwt, plain.logwt)


def test_argument_errors():
    with pytest.raises(ValueError, match="clusterer"):
        run_nested_slice(None, None, 3, seed=1, live=_Runs(MIX), clustering=True, clusterer=cluster_runs, **KW)
    with pytest.raises(ValueError, match="clusterer"):
        run_nested_ensemble(None, None, 3, (1, 2), live=_Runs(MIX), clustering=True, clusterer=cluster_runs, **KW)
    with pytest.raises(ValueError, match="live_chol"):
        run_nested_slice(None, None, 3, seed=1, live=_Runs(MIX), clustering=True, live_chol="host", **KW)
    with pytest.raises(ValueError, match="nboot"):
        run_nested_slice(None, None, 3, seed=1, live=_Runs(MIX), clustering=True, **dict(KW, nboot=33))
    with pytest.raises(ValueError, match="nboot"):
        run_nested_ensemble(None, None, 3, (1, 2), live=_Runs(MIX), clustering=True, **dict(KW, nboot=-1))
    with pytest.raises(ValueError):                          # a live set without the clustered step
        run_nested_slice(None, None, 3, seed=1, live=object(), clustering=True, **KW)
    with pytest.raises(ValueError):
        run_nested_ensemble(None, None, 3, (1, 2), live=_Runs(MIX), clustering=True, walker_runs=MIX.walker_runs, **KW)
