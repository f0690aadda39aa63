"""The resident ensemble (rvll_live_runs_*, GpuRVModel.live_runs_*, nested.run_nested_ensemble(live=model)): R live sets in one
handle, sorted, whitened and walked together, each run bit for bit the standalone resident run of its seed — in the single-kernel
and the rounds forms of the combined walk — with its factors, sorted log-L and dead rows those of its own live_* calls; and the
ensemble's state and the one-run live set refuse each other's calls."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from evidence_amd.nested import run_nested_slice

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


def _same(e, a, s):
    assert e.niter == a.niter and e.ncall == a.ncall, (s, e.niter, a.niter, e.ncall, a.ncall)
    assert e.logz == a.logz and e.logzerr == a.logzerr and e.information == a.information, s
    assert np.array_equal(e.samples, a.samples) and np.array_equal(e.logl, a.logl) and np.array_equal(e.logwt, a.logwt), s


def test_51peg_resident_ensemble_is_the_standalone_resident_runs(gpu_required):
    seeds = (1, 2, 3, 4)
    with _51peg() as m:
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=8_000_000)
        ens = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        # (a one-run resident run on the same model, after the ensemble: its own bits)
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw) for s in seeds]
    for s, e, a in zip(seeds, ens, alone):
        _same(e, a, s)
        assert e.timing["turns"] == e.niter // 100 and e.timing["walk_s"] > 0


def test_51peg_resident_ensemble_in_the_rounds_form(gpu_required):
    # 16 runs x 400 walkers = 6400: the combined walk takes the rounds form, every standalone run's 400 walkers the single kernel
    seeds = tuple(range(101, 117))
    with _51peg() as m:
        kw = dict(nlive=1600, kbatch=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_iter=2000)
        ens = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        rounds = m.slice_walk_rounds()
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw) for s in seeds]
        assert m.slice_walk_rounds() == 0
    assert rounds > 0
    for s, e, a in zip(seeds, ens, alone):
        assert e.niter == 2000
        _same(e, a, s)


def test_gaussian_resident_ensemble(gpu_required):
    """Eight runs of the no-planet Gaussian of test_gpu_ensemble.py (ln Z = -ln 400), resident."""
    seeds = range(11, 19)
    kw = dict(nlive=1000, dlogz=0.01, nsteps=10, max_calls=20_000_000)
    with _gaussian() as m:
        out = run_nested_ensemble(None, None, 2, seeds, live=m, **kw)
        alone = [run_nested_slice(None, None, 2, seed=s, live=m, **kw) for s in seeds]
    assert len(out) == 8
    for s, e, a in zip(seeds, out, alone):
        _same(e, a, s)
        assert abs(e.logz - (-np.log(400.0))) < 4 * e.logzerr + 0.05, (e.logz, e.logzerr)
    assert abs(np.mean([r.logz for r in out]) + np.log(400.0)) < 0.12


def test_factors_sort_and_rows_are_the_one_run_calls(gpu_required):
    R, n, kdead = 5, 400, 100
    runs = np.array([0, 2, 3, 4], dtype=np.int32)         # not every run: the listed ones, packed
    rng = np.random.default_rng(8)
    with _51peg() as m:
        wr = wrapped_params(m.parnames)
        cube = rng.random((R * n, m.ndim))
        logl0 = m.live_runs_init(cube, R)
        got = []
        for it in range(3):                                # three steps: the later ones start from walked rows
            dl, lstar, top = m.live_runs_sort(runs, kdead)
            ranks = rng.integers(0, n - kdead, (runs.size, kdead))
            seeds = [int(v) for v in rng.integers(0, 2 ** 62, runs.size)]
            wl, used, chol = m.live_runs_step(runs, kdead, ranks, lstar, wr, 10, 200, seeds, return_chol=True)
            got.append((dl, lstar, top, ranks, seeds, wl, used, chol))
        rows = [m.live_runs_get(r) for r in range(R)]
        dead = [m.live_runs_dead(r) for r in range(R)]
        assert all(len(dead[r][1]) == (3 * kdead if r in runs else 0) for r in range(R))
        for r in range(R):
            alone_logl = m.live_init(cube[r * n:(r + 1) * n])
            assert np.array_equal(alone_logl, logl0[r])
            if r not in runs:
                assert np.array_equal(rows[r][0], cube[r * n:(r + 1) * n]) and np.array_equal(rows[r][2], logl0[r])
                continue
            a = int(np.flatnonzero(runs == r)[0])
            for dl, lstar, top, ranks, seeds, wl, used, chol in got:
                dl1, lstar1, top1 = m.live_sort(kdead)
                assert np.array_equal(dl[a], dl1) and lstar[a] == lstar1 and top[a] == top1, r
                wl1, used1, chol1 = m.live_step(None, kdead, ranks[a], lstar1, wr, 10, 200, seeds[a], return_chol=True)
                assert np.array_equal(chol[a], chol1) and np.array_equal(wl[a], wl1) and used[a] == used1, r
            u1, th1, ll1 = m.live_get()
            assert np.array_equal(rows[r][0], u1) and np.array_equal(rows[r][1], th1) and np.array_equal(rows[r][2], ll1), r
            dth1, dll1 = m.live_dead()
            assert np.array_equal(dead[r][0], dth1) and np.array_equal(dead[r][1], dll1), r


def test_ensemble_and_one_run_state_refuse_each_other(gpu_required):
    lib = _abi.load()
    R, n, kdead = 3, 200, 50
    rng = np.random.default_rng(2)
    with _gaussian() as m:
        h = m._h
        d = np.empty(kdead)
        ls, tp = C.c_double(), C.c_double()
        m.live_runs_init(rng.random((R * n, 2)), R)
        # the one-run entry points against an ensemble's rows
        assert lib.rvll_live_sort(h, kdead, _abi.as_dp(d), C.byref(ls), C.byref(tp)) == _abi.E_INVALID
        start = np.zeros(kdead, dtype=np.int32)
        nc = C.c_int64()
        assert lib.rvll_live_step(h, None, kdead, _abi.as_ip(start), 0.0, None, None, 4, 200, 1, 0, C.byref(nc),
                                  _abi.as_dp(d), None) == _abi.E_INVALID
        buf = np.empty((R * n, 2))
        assert lib.rvll_live_get(h, _abi.as_dp(buf), None, None) == _abi.E_INVALID
        cnt = C.c_int64(0)
        assert lib.rvll_live_dead(h, C.byref(cnt), None, None) == _abi.E_INVALID
        with pytest.raises(RuntimeError):
            m.live_sort(kdead)
        # ... and the reverse: the ensemble's against a one-run live set
        m.live_init(rng.random((n, 2)))
        runs = np.array([0], dtype=np.int32)
        one, two = np.empty(1), np.empty(1)
        assert lib.rvll_live_runs_sort(h, _abi.as_ip(runs), 1, kdead, _abi.as_dp(d), _abi.as_dp(one), _abi.as_dp(two)) == _abi.E_INVALID
        assert lib.rvll_live_runs_get(h, 0, _abi.as_dp(buf), None, None) == _abi.E_INVALID
        assert lib.rvll_live_runs_dead(h, 0, C.byref(cnt), None, None) == _abi.E_INVALID
        with pytest.raises(RuntimeError):
            m.live_runs_sort([0], kdead)
        dl1, lstar1, _ = m.live_sort(kdead)                 # the one-run set itself still works
        m.live_step(None, kdead, np.zeros(kdead, dtype=np.int32), lstar1, nsteps=4, seed=3)


def test_failed_steps_leave_every_run_as_it_was(gpu_required):
    R, n, kdead = 3, 200, 50
    rng = np.random.default_rng(4)
    runs = np.arange(R, dtype=np.int32)

    def state(m):
        return [(m.live_runs_get(r), m.live_runs_dead(r)) for r in range(R)]

    def same(a, b):
        return all(all(np.array_equal(x, y) for x, y in zip(ga + da, gb + db)) for (ga, da), (gb, db) in zip(a, b))

    def refused(fn):
        with pytest.raises(RvllError) as e:
            fn()
        assert e.value.code == _abi.E_INVALID

    with _gaussian() as m:
        m.live_runs_init(rng.random((R * n, 2)), R)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        ranks = rng.integers(0, n - kdead, (R, kdead))
        m.live_runs_step(runs, kdead, ranks, lstar, None, 4, 200, [1, 2, 3])      # a step in: the dead stores are not empty
        before = state(m)
        # unsorted: no sort since the last step
        refused(lambda: m.live_runs_step(runs, kdead, ranks, lstar, None, 4, 200, [1, 2, 3]))
        assert same(state(m), before)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        # a rank outside the survivors
        bad = ranks.copy()
        bad[1, 7] = n - kdead
        refused(lambda: m.live_runs_step(runs, kdead, bad, lstar, None, 4, 200, [1, 2, 3]))
        assert same(state(m), before)
        # a duplicate run, and runs that differ from the sort's
        refused(lambda: m.live_runs_step([0, 0, 1], kdead, ranks, lstar, None, 4, 200, [1, 2, 3]))
        refused(lambda: m.live_runs_step([0, 1], kdead, ranks[:2], lstar[:2], None, 4, 200, [1, 2]))
        refused(lambda: m.live_runs_sort([1, 0], kdead))
        assert same(state(m), before)
        # an lstar that is not the sort's, and a kdead that is not
        refused(lambda: m.live_runs_step(runs, kdead, ranks, lstar + 1.0, None, 4, 200, [1, 2, 3]))
        refused(lambda: m.live_runs_step(runs, kdead - 1, ranks[:, 1:], lstar, None, 4, 200, [1, 2, 3]))
        assert same(state(m), before)
        # the rows did not move: a new sort finds what the last one found, and its step goes through
        dl2, lstar2, _ = m.live_runs_sort(runs, kdead)
        assert np.array_equal(dl, dl2) and np.array_equal(lstar, lstar2)
        m.live_runs_step(runs, kdead, ranks, lstar2, None, 4, 200, [1, 2, 3])
        after = state(m)
        assert all(len(after[r][1][1]) == 2 * kdead for r in range(R)) and not same(after, before)


@pytest.mark.parametrize("clustered", [False, True], ids=["unclustered", "clustered"])
def test_a_step_that_fails_late_leaves_every_run_as_it_was(gpu_required, clustered):
    """Every refusal of test_failed_steps_leave_every_run_as_it_was happens before anything is touched.  Here the step fails LATE: a
    NaN among run 1's surviving cube rows (Uniform priors: no table lookup sees it) gives a covariance that cannot be factored, after
    the dying rows of all three runs were copied to the dead store.  The store must not count them, no run may get a piece of it, no
    live row and no birth may have changed; and since the failure spent the sort, the other runs step on after a fresh one."""
    R, n, kdead = 3, 200, 50
    rng = np.random.default_rng(6)
    runs = np.arange(R, dtype=np.int32)

    def step(m, which, ranks, lstar, seeds):
        if clustered:
            return m.live_runs_step_clustered(which, kdead, ranks, lstar, None, 4, 200, seeds, 10, [s + 100 for s in seeds])[:2]
        return m.live_runs_step(which, kdead, ranks, lstar, None, 4, 200, seeds)

    def state(m):
        return [m.live_runs_get(r) + m.live_runs_dead(r) + (m.live_runs_dead_count(r),) + m.live_runs_births(r) for r in range(R)]

    def same(a, b):
        return all(np.array_equal(x, y, equal_nan=True) for ra, rb in zip(a, b) for x, y in zip(ra, rb))

    with _gaussian() as m:
        cube = rng.random((R * n, 2))
        m.live_runs_init(cube, R)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        step(m, runs, rng.integers(0, n - kdead, (R, kdead)), lstar, [1, 2, 3])          # a good step: the dead store is in use
        assert all(m.live_runs_dead_count(r) == kdead for r in range(R))
        bad = cube.copy()
        bad[n + 17, 1] = np.nan                                                           # a cube row of run 1
        logl = m.live_runs_init(bad, R)
        assert np.isnan(logl[1, 17]) and np.isfinite(np.delete(logl.ravel(), n + 17)).all()
        before = state(m)
        assert all(s[5] == 0 for s in before)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        assert np.isfinite(dl).all()                                                     # the NaN row sorts last: it survives, so the failure is late
        ranks = rng.integers(0, n - kdead, (R, kdead))
        with pytest.raises(RvllError) as e:
            step(m, runs, ranks, lstar, [4, 5, 6])
        assert e.value.code == _abi.E_INVALID and "positive definite" in str(e.value) and "run 1" in str(e.value), str(e.value)
        assert same(state(m), before)
        two = np.array([0, 2], dtype=np.int32)
        dl2, lstar2, _ = m.live_runs_sort(two, kdead)
        assert np.array_equal(dl2, dl[two]) and np.array_equal(lstar2, lstar[two])
        wl, used = step(m, two, ranks[two], lstar2, [4, 6])
        assert np.isfinite(wl).all() and (np.asarray(used) > 0).all()
        after = state(m)
        assert [s[5] for s in after] == [kdead, 0, kdead]
        assert same([after[1]], [before[1]]) and not same([after[0]], [before[0]]) and not same([after[2]], [before[2]])
