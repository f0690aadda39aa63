"""The step-count adaptation on the GPU: the run-mode walk with one step count per run
(rvll_slice_walk_runs_steps) is every run's own rvll_slice_walk, bit for bit, in every form it takes; the device distances
(rvll_walk_distances_runs) are adapt.py's definition; and an adaptive ensemble on the device walk is its standalone runs."""
import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, adapt, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.nested import run_nested_slice
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _run_starts(m, sizes, seed):
    """Start points of one run per entry of sizes, each with its own lstar, whitening factor and seed
    (tests/test_gpu_ensemble.py's construction)."""
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
        runs.append((cube[:n], theta[:n], logl[:n], lstar, chol, 2000 + 11 * r + seed))
    return runs


def _walk_steps(m, runs, wr, steps):
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])])
    return run_start, m.slice_walk_runs(np.concatenate([r[0] for r in runs]), np.concatenate([r[1] for r in runs]),
                                        np.concatenate([r[2] for r in runs]), run_start, [r[3] for r in runs],
                                        np.stack([r[4] for r in runs]), wr, nsteps=steps, seeds=[r[5] for r in runs])


def _refs(m, runs, wr, steps):
    return [m.slice_walk(c, t, l, ls, ch, wr, nsteps=int(n), seed=s) if len(c) else (c, t, l, 0)
            for (c, t, l, ls, ch, s), n in zip(runs, steps)]


def _assert_runs_equal(run_start, got, ref, what):
    cube, theta, logl, ncalls = got
    for r, (c, t, l, n) in enumerate(ref):
        rows = slice(run_start[r], run_start[r + 1])
        assert np.array_equal(cube[rows], c) and np.array_equal(theta[rows], t) and np.array_equal(logl[rows], l), (what, r)
        assert ncalls[r] == n, (what, r, ncalls[r], n)


SMALL = [700, 1, 0, 600, 699]                     # 2000 walkers
LARGE = [3000, 1, 0, 2500, 2499]                  # 8000 walkers: the rounds form's size
STEPS_SMALL = [3, 250, 17, 1, 40]                 # (the empty run's count is never used)
STEPS_LARGE = [12, 1, 5, 30, 2]


def test_per_run_step_counts_are_each_runs_own_walk(gpu_required, monkeypatch):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        runs = _run_starts(m, SMALL, seed=1)
        ref = _refs(m, runs, wr, STEPS_SMALL)
        run_start, got = _walk_steps(m, runs, wr, STEPS_SMALL)
        _assert_runs_equal(run_start, got, ref, "single kernel")
        assert got[3][1] > 0 and got[3][2] == 0
        # the queue with few slots (two parts: the first part stops short of the long runs), and the full-solver walk
        for env, val in (("RVLL_WALK_QUEUE", "2"), ("RVLL_WALK_FAT", "1")):
            monkeypatch.setenv(env, val)
            ref_e = _refs(m, runs, wr, STEPS_SMALL)
            run_start, got = _walk_steps(m, runs, wr, STEPS_SMALL)
            _assert_runs_equal(run_start, got, ref_e, env)
            monkeypatch.delenv(env)
        # everything deferred by the slim prior stage: the full-solver finish resumes each row up to its own count
        m.set_slim_table_range(0.0)
        ref_d = _refs(m, runs, wr, STEPS_SMALL)
        run_start, got = _walk_steps(m, runs, wr, STEPS_SMALL)
        _assert_runs_equal(run_start, got, ref_d, "deferred")
        m.set_slim_table_range(30.0)
        # at the rounds form's size a mixed table walks in the single-kernel form; a uniform table is the scalar call
        runs = _run_starts(m, LARGE, seed=2)
        ref = _refs(m, runs, wr, STEPS_LARGE)
        run_start, got = _walk_steps(m, runs, wr, STEPS_LARGE)
        assert m.slice_walk_rounds() == 0
        _assert_runs_equal(run_start, got, ref, "large, mixed")
        monkeypatch.setenv("RVLL_WALK_ROUNDS", "1")                     # asked for, the rounds form still steps aside
        run_start, got = _walk_steps(m, runs, wr, STEPS_LARGE)
        assert m.slice_walk_rounds() == 0
        _assert_runs_equal(run_start, got, ref, "large, mixed, rounds asked")
        monkeypatch.delenv("RVLL_WALK_ROUNDS")
        run_start, got = _walk_steps(m, runs, wr, [6] * len(runs))
        rounds = m.slice_walk_rounds()
        scalar = _walk_steps(m, runs, wr, 6)[1]
        assert rounds > 0 and m.slice_walk_rounds() > 0
        for a, b in zip(got, scalar):
            assert np.array_equal(a, b)


def test_per_run_step_count_errors(gpu_required):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        runs = _run_starts(m, [5, 5], seed=3)
        with pytest.raises(ValueError):
            _walk_steps(m, runs, None, [3])
        with pytest.raises(RvllError):
            _walk_steps(m, runs, None, [3, -1])
        with pytest.raises(RvllError):
            _walk_steps(m, runs, None, [3, 1 << 18])


def _offsets_model(ndim):
    """A model with ndim free instrument offsets and no planet (the distances only need the dimension)."""
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    names = [f"i{k}" for k in range(ndim)]
    table = EpochTable.from_arrays(names, np.arange(1.0, ndim + 1.0), np.zeros(ndim), np.ones(ndim), np.arange(ndim))
    pri = {f"{n}_offset": P.Uniform(-10, 10) for n in names}
    return GpuRVModel({}, table, list(pri), priordict=pri)


def _factor(rng, rows, ndim):
    d0 = rows - rows.mean(axis=0) if len(rows) > 1 else rng.random((4, ndim)) - 0.5
    return np.linalg.cholesky(d0.T @ d0 / max(1, len(d0) - 1) + 1e-3 * np.eye(ndim))


@pytest.mark.parametrize("ndim", [3, 12, 64])
def test_device_distances_are_the_definition(gpu_required, ndim):
    rng = np.random.default_rng(50 + ndim)
    sizes = [0, 1, 2, 37, 400, 65, 3]
    groups = [np.clip(rng.normal(rng.random(ndim), 0.1, (n, ndim)), 0.0, np.nextafter(1.0, 0.0)) for n in sizes]
    factors = np.stack([_factor(rng, g, ndim) for g in groups])
    surv = np.concatenate(groups)
    group_start = np.concatenate([[0], np.cumsum(sizes)])
    K = 500
    wg = rng.integers(0, len(sizes), K).astype(np.int32)
    starts = rng.random((K, ndim))
    ends = np.where(rng.random((K, ndim)) < 0.5, starts, rng.random((K, ndim)))
    wr = np.zeros(ndim, dtype=bool)
    wr[::3] = True
    with _offsets_model(ndim) as m:
        for wrapped in (None, wr):
            pair, move = m.walk_distances_runs(surv, group_start, factors, wrapped, starts, ends, wg)
            pair_np, move_np = adapt.walk_distances_runs(surv, group_start, factors, wrapped, starts, ends, wg)
            assert np.array_equal(move, move_np)
            assert np.array_equal(np.isnan(pair), np.isnan(pair_np)) and np.isnan(pair[:2]).all()
            ok = ~np.isnan(pair_np)
            assert np.all(np.abs(pair[ok] - pair_np[ok]) <= 1e-13 * pair_np[ok])
            # every pair distance is the definition's bits: a group of two is its one pair
            assert pair[2] == adapt.dist(groups[2][:1], groups[2][1:], factors[2], wrapped)[0]
            # a group's result does not depend on the others in the call
            alone = m.walk_distances_runs(groups[4], [0, sizes[4]], factors[4:5], wrapped, starts[:0], ends[:0], wg[:0])[0]
            assert alone[0] == pair[4]
        with pytest.raises(ValueError):
            m.walk_distances_runs(surv, group_start, factors, None, starts, ends, np.full(K, len(sizes), dtype=np.int32))
        with pytest.raises(RvllError):
            _raw_bad_group(m, surv, group_start, factors, starts, ends)


def _raw_bad_group(m, surv, group_start, factors, starts, ends):
    """The C entry refuses a walker group outside [0, G) (the binding's own check would raise ValueError first)."""
    import ctypes as C
    from evidence_amd import _abi
    surv = np.ascontiguousarray(surv)
    gs = np.ascontiguousarray(group_start, dtype=np.int64)
    f = np.ascontiguousarray(factors)
    s, e = np.ascontiguousarray(starts[:1]), np.ascontiguousarray(ends[:1])
    wg = np.array([len(gs) - 1], dtype=np.int32)
    pair, move = np.empty(len(gs) - 1), np.empty(1)
    _abi.check(m._lib.rvll_walk_distances_runs(m._h, _abi.as_dp(surv), gs.ctypes.data_as(C.POINTER(C.c_int64)), len(gs) - 1,
                                               _abi.as_dp(f), None, _abi.as_dp(s), _abi.as_dp(e), _abi.as_ip(wg), 1,
                                               _abi.as_dp(pair), _abi.as_dp(move)))


@pytest.mark.parametrize("clustering", [False, True])
def test_adaptive_ensemble_on_the_device_is_the_standalone_runs(gpu_required, clustering):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=120, kbatch=30, nsteps=4, dlogz=0.5, max_iter=3000, wrapped=wr, clustering=clustering,
                  adaptive_nsteps="move-distance", min_nsteps=1, max_nsteps=40)
        if clustering:
            kw["clusterer"] = m.cluster_runs
        seeds = [3, 4, 5]
        got = run_nested_ensemble(prior, loglike, m.ndim, seeds, walker_runs=m.slice_walk_runs, distances=m.walk_distances_runs, **kw)
        assert all(len(g.nsteps_trace) > 0 for g in got)
        assert len({tuple(g.nsteps_trace) for g in got}) > 1            # the runs took different step counts
        for s, g in zip(seeds, got):
            one = run_nested_slice(prior, loglike, m.ndim, seed=s, walker_runs=m.slice_walk_runs,
                                   distances=m.walk_distances_runs, **kw)
            assert g.niter == one.niter and g.ncall == one.ncall and g.logz == one.logz
            assert np.array_equal(g.samples, one.samples) and np.array_equal(g.logl, one.logl)
            assert np.array_equal(g.nsteps_trace, one.nsteps_trace)
            assert np.array_equal(g.far_fraction, one.far_fraction, equal_nan=True)


# ---- the resident ensemble ---------------------------------------------------------------------------------------------
def _resident_step(m, kdead, steps, seed, **kw):
    """One sort + step of every run of m's resident ensemble; returns what the step returns and the rows before it."""
    runs = np.arange(kw.pop("R"))
    before = [m.live_runs_get(int(r)) for r in runs]
    dl, lstar, top = m.live_runs_sort(runs, kdead)
    rng = np.random.default_rng(seed)
    n = before[0][0].shape[0]
    ranks = rng.integers(0, n - kdead, (runs.size, kdead))
    seeds = [int(s) for s in rng.integers(0, 2 ** 62, runs.size)]
    return before, lstar, m.live_runs_step(runs, kdead, ranks, lstar, kw.get("wrapped"), steps, 200, seeds, **kw.get("extra", {}))


def test_resident_step_table_uniform_is_the_scalar_step_and_distances_fit(gpu_required):
    w = make_workload(3)
    R, n, kdead = 4, 200, 40
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        cube = np.random.default_rng(7).random((R * n, m.ndim))
        outs = []
        for steps in (5, [5] * R):                       # the old entry, then the step table (uniform, no distances)
            m.live_runs_init(cube, R)
            got = []
            for it in range(3):
                got.append(_resident_step(m, kdead, steps, 100 + it, R=R, wrapped=wr)[2])
            outs.append((got, [m.live_runs_get(r) for r in range(R)]))
        for (a, b) in zip(outs[0][0], outs[1][0]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for a, b in zip(outs[0][1], outs[1][1]):
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
        # a mixed table with distances: every run's pair is the mean pair distance of its survivors under its factor
        m.live_runs_init(cube, R)
        before, lstar, (wl, used, move, pair) = _resident_step(m, kdead, [1, 7, 3, 12], 5, R=R, wrapped=wr,
                                                                extra={"return_distances": True})
        assert move.shape == pair.shape == (R, kdead) and np.all(move >= 0)
        for r in range(R):
            surv = before[r][0][before[r][2] > lstar[r]]
            d0 = surv - surv.mean(axis=0)
            L = np.linalg.cholesky(d0.T @ d0 / (len(surv) - 1) + 1e-14 * np.eye(m.ndim))
            want = adapt.pair_mean(surv, L, wr)
            assert np.all(pair[r] == pair[r, 0]) and abs(pair[r, 0] - want) <= 1e-6 * want, (r, pair[r, 0], want)


@pytest.mark.parametrize("clustering", [False, True])
def test_resident_adaptive_ensemble_is_the_standalone_runs(gpu_required, clustering):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        wr = wrapped_params(m.parnames)
        kw = dict(nlive=120, kbatch=30, nsteps=4, dlogz=0.5, max_iter=3000, wrapped=wr, clustering=clustering)
        plain = run_nested_ensemble(None, None, m.ndim, [6, 7], live=m, **kw)
        pinned = run_nested_ensemble(None, None, m.ndim, [6, 7], live=m, adaptive_nsteps="move-distance", max_nsteps=4, **kw)
        for a, b in zip(plain, pinned):                  # a pinned table (with the distances returned) is the plain step
            assert a.niter == b.niter and a.ncall == b.ncall and a.logz == b.logz
            assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl)
            assert np.all(b.nsteps_trace == 4) and b.far_fraction.shape == b.nsteps_trace.shape
        seeds = [3, 4, 5]
        kw.update(adaptive_nsteps="move-distance", min_nsteps=1, max_nsteps=40)
        got = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        assert len({tuple(g.nsteps_trace) for g in got}) > 1
        for s, g in zip(seeds, got):
            one = run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw)
            assert g.niter == one.niter and g.ncall == one.ncall and g.logz == one.logz
            assert np.array_equal(g.samples, one.samples) and np.array_equal(g.logl, one.logl)
            assert np.array_equal(g.logl_birth, one.logl_birth)
            assert np.array_equal(g.nsteps_trace, one.nsteps_trace)
            assert np.array_equal(g.far_fraction, one.far_fraction, equal_nan=True)
