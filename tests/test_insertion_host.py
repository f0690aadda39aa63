"""CPU: birth contours in the host drivers' results, and the insertion-index test (evidence_amd/insertion.py) — its definition
against a simulated sampler that records each new point's rank when it is inserted, against a brute-force count on hand-built
rows, and the KS records it gives for perfect and truncated samplers."""
import numpy as np
import pytest

from evidence_amd import _abi, insertion, run_nested_ensemble
from evidence_amd.nested import NestedResult, run_nested, run_nested_slice
from tests.insertion_sim import simulate
from tests.test_nested_ensemble_host import KW, loglike, prior


def _result(logl, birth, nlive):
    n = len(logl)
    return NestedResult(0.0, 0.0, 0, 0, 0.0, np.zeros((n, 1)), logl, np.zeros(n), nlive=nlive, logl_birth=birth)


def _brute(logl, birth, run_start):
    """The definition, one row and one candidate at a time."""
    index = np.full(len(logl), -1, dtype=np.int64)
    n_at = np.full(len(logl), -1, dtype=np.int64)
    for r in range(len(run_start) - 1):
        rows = range(run_start[r], run_start[r + 1])
        for j in rows:
            b = birth[j]
            if b == -np.inf:
                continue
            live = [k for k in rows if birth[k] <= b and logl[k] > b]
            n_at[j] = len(live)
            index[j] = sum(1 for k in live if logl[k] < logl[j])
    return index, n_at


@pytest.mark.parametrize("kbatch,niter", [(1, 3000), (25, 120)])
def test_definition_recovers_the_simulated_ranks(kbatch, niter):
    for seed in (1, 2):
        logl, birth, rank = simulate(100, kbatch, niter, seed)
        index, n_at = insertion.indexes_arrays(logl, birth, [0, len(logl)])
        ins = birth > -np.inf
        assert np.count_nonzero(ins) == kbatch * niter
        assert np.array_equal(index[ins], rank[ins])
        assert np.all(n_at[ins] == 100)
        assert np.all(index[~ins] == -1) and np.all(n_at[~ins] == -1)
        # any row order, and one call for several runs, give the same per-row answer
        perm = np.random.default_rng(seed).permutation(len(logl))
        i2, n2 = insertion.indexes_arrays(np.concatenate([logl, logl[perm]]), np.concatenate([birth, birth[perm]]),
                                          [0, len(logl), 2 * len(logl)])
        assert np.array_equal(i2[:len(logl)], index) and np.array_equal(i2[len(logl):], index[perm])
        assert np.array_equal(n2[len(logl):], n_at[perm])


@pytest.mark.parametrize("kbatch", [1, 25])
def test_a_perfect_sampler_passes(kbatch):
    for seed in (3, 4, 5):
        logl, birth, _ = simulate(100, kbatch, 5000 // kbatch, seed)
        out = insertion.test([_result(logl, birth, 100)])
        rec = out["runs"][0]
        assert rec["n"] == 5000 and rec["off_schedule"] == 0 and rec["off_contour"] == 0
        assert rec["pvalue"] > 0.01 and not rec["failed"] and rec["first_window"] is None
        assert rec["windows"] == 50 and out["pooled"]["n"] == 5000


def test_a_truncated_sampler_fails():
    logl, birth, _ = simulate(100, 1, 5000, 6, reach=lambda it: 0.9)
    rec = insertion.test([_result(logl, birth, 100)])["runs"][0]
    assert rec["pvalue"] < 1e-10 and rec["failed"]


def test_the_first_failing_window_is_where_the_sampler_breaks():
    niter = 6000
    logl, birth, _ = simulate(100, 1, niter, 7, reach=lambda it: 1.0 if it < niter // 2 else 0.85)
    rec = insertion.test([_result(logl, birth, 100)])["runs"][0]
    assert rec["failed"] and rec["first_window"] is not None
    assert rec["first_window"] >= rec["windows"] // 2
    assert rec["first_window_deaths"] >= niter // 2
    assert rec["first_window_birth"] == np.sort(logl)[rec["first_window_deaths"] - 1]


def test_hand_built_rows_match_a_brute_force_count():
    rng = np.random.default_rng(8)
    runs = []
    # ties everywhere: values on a coarse grid, births among them
    ll = rng.integers(-5, 5, 60).astype(np.float64)
    bb = np.where(rng.random(60) < 0.3, -np.inf, rng.integers(-6, 4, 60).astype(np.float64))
    runs.append((ll, bb))
    # a -1e30 plateau: rows born on it, rows at it, -0.0 and +0.0 mixed
    ll = np.concatenate([np.full(10, -1e30), rng.normal(size=30), [0.0, -0.0, 0.0]])
    bb = np.concatenate([np.full(10, -np.inf), np.full(15, -1e30), np.full(15, -np.inf), [-0.0, 0.0, -1e30]])
    runs.append((ll, bb))
    # off-contour rows (logl <= birth) among a simulated run, rows shuffled (final live rows unsorted, dead rows out of order)
    logl, birth, _ = simulate(30, 3, 40, 9)
    pick = rng.choice(np.flatnonzero(birth > -np.inf), 6, replace=False)
    logl[pick[:3]] = birth[pick[:3]]
    logl[pick[3:]] = birth[pick[3:]] - 0.01
    perm = rng.permutation(len(logl))
    runs.append((logl[perm], birth[perm]))
    runs.append((np.array([1.0]), np.array([-np.inf])))          # no deaths at all
    runs.append((np.array([2.0, 3.0]), np.array([np.inf, 2.0])))   # a birth at +inf: an empty live set
    logl = np.concatenate([r[0] for r in runs])
    birth = np.concatenate([r[1] for r in runs])
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])])
    index, n_at = insertion.indexes_arrays(logl, birth, run_start)
    bi, bn = _brute(logl, birth, run_start)
    assert np.array_equal(index, bi) and np.array_equal(n_at, bn)
    offc = (birth > -np.inf) & (logl <= birth)
    assert np.all(index[offc] == 0)


def test_records_count_off_contour_and_off_schedule_rows():
    logl, birth, _ = simulate(50, 5, 100, 10)
    logl[200] = birth[200]                                        # an end point lowered onto its contour
    birth[300:305] = birth[299]                                   # rows born on a contour shared with other batches
    rec = insertion.test([_result(logl, birth, 50)])["runs"][0]
    assert rec["off_contour"] == 1 and rec["off_schedule"] > 0
    assert rec["n"] + rec["off_contour"] + rec["off_schedule"] == np.count_nonzero(birth > -np.inf)


def test_bad_input_is_refused():
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, np.nan], [-np.inf, 0.0], [0, 2])
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, 2.0], [-np.inf, np.nan], [0, 2])
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, 2.0], [-np.inf, 0.0], [0, 1])
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, 2.0], [-np.inf, 0.0], [0])
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, 2.0], [-np.inf, 0.0], [0, 2, 1, 2])


def test_a_result_without_births_is_refused():
    res = _result(np.array([1.0, 2.0]), None, 2)
    with pytest.raises(ValueError):
        insertion.test([res])
    with pytest.raises(ValueError):
        insertion.indexes([res])


def _check_births(res, nlive, kbatch):
    """The invariants every host driver's births keep."""
    birth, logl = res.logl_birth, res.logl
    assert birth.shape == logl.shape and birth.dtype == np.float64
    ndead = res.niter
    tops = logl[kbatch - 1:ndead:kbatch]                          # each batch's highest dying log-L
    fin = birth > -np.inf
    assert np.count_nonzero(~fin) == nlive                        # the initial live points
    assert np.all(np.isin(birth[fin], tops))
    assert np.all(birth[fin] < logl[fin])                         # the host walks accept on the log-L they return
    index, n_at = insertion.indexes([res])[0]
    assert np.all(n_at[fin] == nlive)
    rec = insertion.test([res])["runs"][0]
    assert rec["off_contour"] == 0 and rec["off_schedule"] == 0 and rec["n"] == np.count_nonzero(fin)


def test_run_nested_records_births():
    res = run_nested(prior, loglike, 2, nlive=80, dlogz=0.5, seed=3)
    _check_births(res, 80, 1)


def test_run_nested_slice_records_births():
    res = run_nested_slice(prior, loglike, 2, seed=4, **KW)
    _check_births(res, KW["nlive"], KW["kbatch"])
    res = run_nested_slice(prior, loglike, 2, seed=4, walker=_draw, **KW)
    _check_births(res, KW["nlive"], KW["kbatch"])


def test_run_nested_slice_clustered_records_births():
    res = run_nested_slice(prior, loglike, 2, seed=5, clustering=True, **KW)      # (the host's own slice walk, per cluster)
    _check_births(res, KW["nlive"], KW["kbatch"])


def _draw(cube, theta, logl, lstar, chol, wrapped, nsteps, max_rounds, seed):
    """A walker that draws every end point from the prior restricted to logL > lstar (rejection from the whole cube): a
    perfect sampler that always moves, deterministic by seed."""
    rng = np.random.default_rng(seed)
    c = cube.copy()
    todo, used = np.arange(len(c)), 0
    while todo.size:
        prop = rng.random((todo.size, c.shape[1]))
        ok = loglike(prior(prop)) > lstar
        c[todo[ok]] = prop[ok]
        used += todo.size
        todo = todo[~ok]
    th = prior(c)
    return c, th, loglike(th), used


def _draw_runs(cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
    out = [np.empty_like(cube), np.empty_like(theta), np.empty_like(logl)]
    ncalls = np.zeros(len(run_start) - 1, dtype=np.int64)
    for r in range(len(run_start) - 1):
        rows = slice(run_start[r], run_start[r + 1])
        c, t, l, ncalls[r] = _draw(cube[rows], theta[rows], logl[rows], lstar[r], chol[r], wrapped, nsteps, max_rounds, seeds[r])
        out[0][rows], out[1][rows], out[2][rows] = c, t, l
    return out[0], out[1], out[2], ncalls


def test_host_ensemble_births_are_the_standalone_runs():
    seeds = [11, 12, 13]
    got = run_nested_ensemble(prior, loglike, 2, seeds, walker_runs=_draw_runs, **KW)
    for s, res in zip(seeds, got):
        alone = run_nested_slice(prior, loglike, 2, seed=s, walker=_draw, **KW)
        assert np.array_equal(res.logl, alone.logl)
        assert np.array_equal(res.logl_birth, alone.logl_birth)
        _check_births(res, KW["nlive"], KW["kbatch"])
    out = insertion.test(got)
    assert len(out["runs"]) == 3 and out["pooled"]["n"] == sum(r["n"] for r in out["runs"])
    assert not out["pooled"]["failed"]


def test_the_library_exports_the_new_symbols():
    import ctypes as C
    lib = C.CDLL(str(_abi.LIB_PATH))
    for name in ("rvll_live_births", "rvll_live_runs_births", "rvll_insertion_indexes"):
        assert hasattr(lib, name), name
    major, minor = C.c_int32(), C.c_int32()
    lib.rvll_version(C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == _abi.ABI_VERSION == (0, 8)
