"""The walks of many independent runs in one device walk (rvll_slice_walk_runs, GpuRVModel.slice_walk_runs) and the
lockstep driver on top of it (nested.run_nested_ensemble): every run's end points, theta, log-L and call count are those of
its own rvll_slice_walk, bit for bit, in every form the walk takes; the ensemble of nested-sampling runs is the standalone
runs; and its evidences sit on an analytic answer."""
import numpy as np
import pytest

from evidence_amd import GpuRVModel, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.nested import run_nested_slice
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def _run_starts(m, sizes, seed):
    """Start points of one run per entry of sizes: each with its own lstar (a different quantile of a prior sample),
    whitening factor (of its own survivors) and seed."""
    rng = np.random.default_rng(seed)
    runs = []
    for r, n in enumerate(sizes):
        q = 0.3 + 0.1 * (r % 5)
        cube = rng.random((int(n / (1 - q)) + 64, m.ndim))
        theta, logl = m.prior_loglike_batch(cube)
        lstar = float(np.quantile(logl, q))
        keep = logl > lstar
        cube, theta, logl = cube[keep], theta[keep], logl[keep]
        d0 = cube - cube.mean(axis=0)
        chol = np.linalg.cholesky(d0.T @ d0 / (len(cube) - 1) + 1e-14 * np.eye(m.ndim))
        runs.append((cube[:n], theta[:n], logl[:n], lstar, chol, 1000 + 7 * r + seed))
    return runs


def _walk_both(m, runs, wr, nsteps):
    """The runs through one slice_walk_runs, and each through its own slice_walk."""
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])])
    got = m.slice_walk_runs(np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]),
                            np.concatenate([r[2] for r in runs]), run_start, [r[3] for r in runs], np.stack([r[4] for r in runs]),
                            wr, nsteps=nsteps, seeds=[r[5] for r in runs])
    rounds = m.slice_walk_rounds()
    ref = [m.slice_walk(c, t, l, ls, ch, wr, nsteps=nsteps, seed=s) if len(c) else (c, t, l, 0) for c, t, l, ls, ch, s in runs]
    return run_start, got, rounds, ref


def _assert_runs_equal(run_start, got, ref, what):
    cube, theta, logl, ncalls = got
    assert len(ncalls) == len(ref)
    for r, (c, t, l, n) in enumerate(ref):
        rows = slice(run_start[r], run_start[r + 1])
        assert np.array_equal(cube[rows], c) and np.array_equal(theta[rows], t) and np.array_equal(logl[rows], l), (what, r)
        assert ncalls[r] == n, (what, r, ncalls[r], n)


# runs of different sizes, a run of one walker and an empty run among them
SMALL = [700, 1, 0, 600, 699]                     # 2000 walkers: the single-kernel form
LARGE = [3000, 1, 0, 2500, 2499]                  # 8000 walkers: the rounds form


def test_runs_walk_is_the_runs_walked_one_by_one(gpu_required):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        runs = _run_starts(m, SMALL, seed=1)
        run_start, got, rounds, ref = _walk_both(m, runs, wr, nsteps=9)
        assert rounds == 0
        _assert_runs_equal(run_start, got, ref, "single kernel")
        assert (got[2][run_start[0]:run_start[1]] > runs[0][3]).all() and got[3][2] == 0
        # the runs are not one run: each walked inside its own lstar with its own factor and seed
        assert len({r[3] for r in runs}) == len(runs)
        runs = _run_starts(m, LARGE, seed=2)
        run_start, got, rounds, ref = _walk_both(m, runs, wr, nsteps=6)
        assert rounds > 0
        _assert_runs_equal(run_start, got, ref, "rounds")


def test_runs_walk_with_deferred_walkers_and_the_full_solvers(gpu_required, monkeypatch):
    """The walkers the slim prior stage defers are finished by the full-solver walk, in run mode as in the one-run walk:
    everything deferred (table range 0), in the single-kernel form and in the rounds form; and the full-solver walk alone."""
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        small, large = _run_starts(m, SMALL, seed=3), _run_starts(m, LARGE, seed=4)
        monkeypatch.setenv("RVLL_WALK_FAT", "1")
        run_start, got, rounds, ref = _walk_both(m, small, wr, nsteps=5)
        _assert_runs_equal(run_start, got, ref, "fat")
        monkeypatch.delenv("RVLL_WALK_FAT")
        # few workgroups: the rows go through the queue, in two parts (the second dealt by what the first cost)
        monkeypatch.setenv("RVLL_WALK_QUEUE", "2")
        run_start, got, rounds, ref = _walk_both(m, small, wr, nsteps=9)
        _assert_runs_equal(run_start, got, ref, "queue, two parts")
        monkeypatch.delenv("RVLL_WALK_QUEUE")
        m.set_slim_table_range(0.0)
        run_start, got, rounds, ref = _walk_both(m, small, wr, nsteps=5)
        _assert_runs_equal(run_start, got, ref, "deferred, single kernel")
        monkeypatch.setenv("RVLL_WALK_ROUNDS", "1")
        run_start, got, rounds, ref = _walk_both(m, large, wr, nsteps=4)
        assert rounds > 0
        _assert_runs_equal(run_start, got, ref, "deferred, rounds")
        monkeypatch.delenv("RVLL_WALK_ROUNDS")
        m.set_slim_table_range(30.0)
        monkeypatch.setenv("RVLL_WALK_ROWS", "1")                       # the rows forms have no run mode: refused
        from evidence_amd import RvllError
        with pytest.raises(RvllError):
            m.slice_walk_runs(small[0][0], small[0][1], small[0][2], [0, len(small[0][0])], [small[0][3]], small[0][4][None],
                              wr, nsteps=3, seeds=[1])


def test_runs_walk_with_walkers_ending_on_a_wandering_solve(gpu_required):
    """The exact redo of the log-L of walkers that end on a wandering Kepler solve (test_gpu_walk.py) in run mode."""
    import golden
    from evidence_amd import priors as P
    case = golden.high_ecc_case()
    lo, hi = case.theta.min(axis=0), case.theta.max(axis=0)
    pri = {n: P.Uniform(float(a), float(b if b > a else a + 1.0)) for n, a, b in zip(case.parnames, lo, hi)}
    pri["planet1_ecc"] = P.Uniform(0.95, 0.9925)
    with GpuRVModel(case.fixed, case.table, case.parnames, priordict=pri) as m:
        wr = wrapped_params(m.parnames)
        runs = _run_starts(m, [900, 1, 0, 1100], seed=5)
        run_start, got, rounds, ref = _walk_both(m, runs, wr, nsteps=6)
        _assert_runs_equal(run_start, got, ref, "wandering")
        flags = m.log_likelihood_batch(m.prior_transform_batch(got[0]), return_flags=True)[1]
        assert ((flags & 4) != 0).sum() > 0
        th_chk, ll_chk = m.prior_loglike_batch(got[0])
        assert np.array_equal(th_chk, got[1]) and np.array_equal(ll_chk, got[2])


def test_runs_walk_argument_errors(gpu_required):
    w = make_workload(1)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        c, t, l, ls, ch, s = _run_starts(m, [50], seed=6)[0]
        with pytest.raises(ValueError):
            m.slice_walk_runs(c, t, l, [0, 40], [ls], ch[None], seeds=[s])                 # run_start does not end at K
        with pytest.raises(ValueError):
            m.slice_walk_runs(c, t, l, [0, 30, 20, 50], [ls] * 3, np.stack([ch] * 3), seeds=[s] * 3)   # decreasing
        with pytest.raises(ValueError):
            m.slice_walk_runs(c, t, l, [0, 50], [ls], ch, seeds=[s])                       # chol not [R, ndim, ndim]
        with pytest.raises(ValueError):
            m.slice_walk_runs(c, t, l, [0, 50], [ls, ls], ch[None], seeds=[s])             # lstar per run
        out = m.slice_walk_runs(c, t, l, [0, 50], [ls], ch[None], nsteps=0, seeds=[s])
        assert np.array_equal(out[0], c) and list(out[3]) == [0]


def test_51peg_ensemble_is_the_standalone_runs(gpu_required):
    from pathlib import Path
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    seeds = (1, 2, 3, 4)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=8_000_000)
        ens = run_nested_ensemble(prior, loglike, m.ndim, seeds, walker_runs=m.slice_walk_runs, **kw)
        alone = [run_nested_slice(prior, loglike, m.ndim, seed=s, walker=m.slice_walk, **kw) for s in seeds]
    for s, e, a in zip(seeds, ens, alone):
        assert e.niter == a.niter and e.ncall == a.ncall, s
        assert e.logz == a.logz and e.logzerr == a.logzerr and e.information == a.information, s
        assert np.array_equal(e.samples, a.samples) and np.array_equal(e.logl, a.logl) and np.array_equal(e.logwt, a.logwt), s


def test_gaussian_evidence_of_an_ensemble(gpu_required):
    """Eight runs of the no-planet Gaussian of test_gpu_walk.py (ln Z = -ln 400) through one ensemble."""
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    table = EpochTable.from_arrays(["a", "b"], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], [0, 1])
    pri = {"a_offset": P.Uniform(-10, 10), "b_offset": P.Uniform(-10, 10)}
    with GpuRVModel({}, table, list(pri), priordict=pri) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        out = run_nested_ensemble(prior, loglike, 2, range(11, 19), nlive=1000, dlogz=0.01, nsteps=10,
                                  max_calls=20_000_000, walker_runs=m.slice_walk_runs)
    assert len(out) == 8
    for r in out:
        assert abs(r.logz - (-np.log(400.0))) < 4 * r.logzerr + 0.05, (r.logz, r.logzerr)
    assert abs(np.mean([r.logz for r in out]) + np.log(400.0)) < 0.12
