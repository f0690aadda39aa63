"""Clustering inside the resident ensemble (rvll_live_runs_step_clustered, GpuRVModel.live_runs_step_clustered):
the step's labels are clustering.cluster_runs of the downloaded survivors, its per-cluster factors those of numpy, its walk
rvll_slice_walk_runs on the same groups; a clustered resident ensemble is its standalone runs, a unimodal run is the
unclustered resident run, and refused steps leave every run as it was."""
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from evidence_amd.clustering import cluster_runs as np_cluster_runs
from evidence_amd.nested import _covariance, _walk_groups, _whitening, run_nested_slice

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _51peg():
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def _gaussian():
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    table = EpochTable.from_arrays(["a", "b"], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], [0, 1])
    pri = {"a_offset": P.Uniform(-10, 10), "b_offset": P.Uniform(-10, 10)}
    return GpuRVModel({}, table, list(pri), priordict=pri)


def _close(got, ref, rel=1e-10):
    assert np.max(np.abs(got - ref)) <= rel * np.max(np.abs(ref)), np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def _same(e, a, s):
    assert e.niter == a.niter and e.ncall == a.ncall, (s, e.niter, a.niter, e.ncall, a.ncall)
    assert e.logz == a.logz and e.logzerr == a.logzerr and e.information == a.information, s
    assert np.array_equal(e.samples, a.samples) and np.array_equal(e.logl, a.logl) and np.array_equal(e.logwt, a.logwt), s


def test_51peg_clustered_steps_are_numpy_clusters_factors_and_the_walk(gpu_required):
    R, n, kdead, nboot, nsteps = 4, 400, 100, 30, 10
    runs = np.array([0, 2, 3], dtype=np.int32)           # not every run: the listed ones, packed
    rng = np.random.default_rng(21)
    checked = {"multi": 0, "own": 0, "global": 0}
    with _51peg() as m:
        wr = wrapped_params(m.parnames)
        D = m.ndim
        cube = rng.random((R * n, D))
        m.live_runs_init(cube, R)
        idle = m.live_runs_get(1)
        for it in range(40):
            before = [m.live_runs_get(r) for r in runs]
            dl, lstar, top = m.live_runs_sort(runs, kdead)
            ranks = rng.integers(0, n - kdead, (runs.size, kdead))
            seeds = [int(v) for v in rng.integers(0, 2 ** 62, runs.size)]
            boots = [int(v) for v in rng.integers(0, 2 ** 63, runs.size)]
            wl, used, ncl = m.live_runs_step_clustered(runs, kdead, ranks, lstar, wr, nsteps, 200, seeds, nboot, boots)
            after = [m.live_runs_get(r) for r in runs]
            for a in range(runs.size):
                u, th, ll = before[a]
                order = np.argsort(ll, kind="stable")
                dead, alive = order[:kdead], order[kdead:]
                ua = u[alive]
                labels, scale, factors = m.live_runs_clusters(a)
                k = int(ncl[a])
                # 1. the metric of the step's global covariance, and the labels of the survivors in rank order, bit for bit
                _close(scale, 1.0 / np.sqrt(np.diag(_covariance(ua))))
                lab_ref, ncl_ref, _ = np_cluster_runs(ua, [0, len(ua)], scale[None, :], wr, nboot, [boots[a]])
                assert np.array_equal(labels, lab_ref) and k == int(ncl_ref[0]), (it, a)
                # 2. every cluster's factor: its own rows' (2 ndim rows or more), else the run's global one
                assert factors.shape == (max(k, 1), D, D)
                glob = _whitening(ua)
                if k <= 1:
                    _close(factors[0], glob)
                else:
                    checked["multi"] += 1
                    small = [c for c in range(k) if np.count_nonzero(labels == c) < 2 * D]
                    for c in range(k):
                        if c in small:
                            _close(factors[c], glob)
                            assert np.array_equal(factors[c], factors[small[0]])
                            checked["global"] += 1
                        else:
                            _close(factors[c], _whitening(ua[labels == c]))
                            checked["own"] += 1
                # 3. the new rows and calls are slice_walk_runs on the same start rows, groups, factors and seeds
                st = alive[ranks[a]]
                wo, sizes, gf, gseeds = _walk_groups(labels[ranks[a]].astype(np.intp), list(factors), seeds[a])
                run_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
                gu, gt, gl, gcalls = m.slice_walk_runs(u[st][wo], th[st][wo], ll[st][wo], run_start, np.full(len(sizes), lstar[a]),
                                                       np.stack(gf), wr, nsteps, 200, gseeds)
                assert np.array_equal(wl[a][wo], gl) and used[a] == int(np.sum(gcalls)), (it, a)
                u2, th2, ll2 = after[a]
                back = dead[wo]
                assert np.array_equal(u2[back], gu) and np.array_equal(th2[back], gt) and np.array_equal(ll2[back], gl)
                keep = np.setdiff1d(np.arange(n), dead)
                assert np.array_equal(u2[keep], u[keep]) and np.array_equal(ll2[keep], ll[keep])
        assert all(np.array_equal(x, y) for x, y in zip(m.live_runs_get(1), idle))        # an unlisted run does not move
        assert all(m.live_runs_dead_count(r) == (40 * kdead if r in runs else 0) for r in range(R))
        ph = m.live_runs_cluster_phases()
        assert all(v > 0 for v in ph.values()), ph
    assert checked["multi"] > 0 and checked["own"] > 0, checked


def test_51peg_clustered_resident_ensemble_is_the_standalone_runs(gpu_required):
    seeds = (1, 2, 3)
    with _51peg() as m:
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=8_000_000, clustering=True)
        ens = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw) for s in seeds]
    for s, e, a in zip(seeds, ens, alone):
        _same(e, a, s)
        assert np.array_equal(e.nclusters, a.nclusters) and len(e.nclusters) == e.niter // 100, s
        assert e.timing["turns"] == e.niter // 100
    assert max(int(np.max(e.nclusters)) for e in ens) >= 2


def test_unimodal_gaussian_resident_clustered_is_unclustered(gpu_required):
    kw = dict(nlive=1000, dlogz=0.01, nsteps=10, max_calls=20_000_000)
    with _gaussian() as m:
        on = run_nested_slice(None, None, 2, seed=1, live=m, clustering=True, **kw)
        off = run_nested_slice(None, None, 2, seed=1, live=m, **kw)
    assert len(on.nclusters) > 0 and np.all(on.nclusters == 1)
    _same(on, off, 1)
    assert abs(on.logz + np.log(400.0)) < 4 * on.logzerr + 0.05


def test_refused_clustered_steps_leave_every_run_as_it_was(gpu_required):
    R, n, kdead = 3, 200, 50
    rng = np.random.default_rng(4)
    runs = np.arange(R, dtype=np.int32)
    boots = [7, 8, 9]

    def state(m):
        return [(m.live_runs_get(r), m.live_runs_dead(r)) for r in range(R)]

    def same(a, b):
        return all(all(np.array_equal(x, y) for x, y in zip(ga + da, gb + db)) for (ga, da), (gb, db) in zip(a, b))

    def refused(fn):
        with pytest.raises(RvllError) as e:
            fn()
        assert e.value.code == _abi.E_INVALID

    def step(m, ranks, lstar, nboot=30, kd=kdead):
        return m.live_runs_step_clustered(runs, kd, ranks, lstar, None, 4, 200, [1, 2, 3], nboot, boots)

    with _gaussian() as m:
        m.live_runs_init(rng.random((R * n, 2)), R)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        ranks = rng.integers(0, n - kdead, (R, kdead))
        step(m, ranks, lstar)                               # a step in: the dead stores are not empty
        before = state(m)
        refused(lambda: step(m, ranks, lstar))             # no sort since the last step
        assert same(state(m), before)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        bad = ranks.copy()
        bad[1, 7] = n - kdead
        refused(lambda: step(m, bad, lstar))               # a rank outside the survivors
        assert same(state(m), before)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        refused(lambda: step(m, ranks, lstar + 1.0))       # an lstar that is not the sort's
        assert same(state(m), before)
        for nb in (33, -1):                                 # nboot outside [0, 32]
            dl, lstar, _ = m.live_runs_sort(runs, kdead)
            refused(lambda: step(m, ranks, lstar, nboot=nb))
            assert same(state(m), before)
        dl2, lstar2, _ = m.live_runs_sort(runs, kdead)      # the rows did not move: a new sort finds what the last one found
        assert np.array_equal(dl, dl2) and np.array_equal(lstar, lstar2)
        _wl, _used, ncl = step(m, ranks, lstar2)
        after = state(m)
        assert all(len(after[r][1][1]) == 2 * kdead for r in range(R)) and not same(after, before)
        assert ncl.shape == (R,) and np.all(ncl >= 1)
