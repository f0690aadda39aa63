"""Insertion indexes on the GPU (rvll_insertion_indexes; insertion.indexes_arrays(device=0)) against the numpy definition on
ragged synthetic runs, and the birth contours the resident live sets record (rvll_live_births, rvll_live_runs_births): those of
the standalone runs and of the host-managed walk, the invariants of a correct sampler, and a refused step leaves them as they
were."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, insertion, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.nested import run_nested_slice
from evidence_amd.synthetic import make_workload
from tests.insertion_sim import simulate

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


def _ragged_runs():
    """Runs of every kind the kernel must get right."""
    rng = np.random.default_rng(21)
    runs = []
    for k, (nlive, kbatch, niter) in enumerate([(100, 1, 900), (100, 25, 40), (1000, 250, 6), (70, 7, 60), (500, 1, 300)]):
        logl, birth, _ = simulate(nlive, kbatch, niter, 30 + k)               # bands up to nlive long: many waves per row
        runs.append((logl, birth))
    runs.append((rng.normal(size=40), np.full(40, -np.inf)))                  # no deaths
    ll = rng.integers(-5, 5, 300).astype(np.float64)                          # ties everywhere
    bb = np.where(rng.random(300) < 0.2, -np.inf, rng.integers(-6, 4, 300).astype(np.float64))
    runs.append((ll, bb))
    ll = np.concatenate([np.full(50, -1e30), rng.normal(size=200), [0.0, -0.0, 0.0, -0.0]])   # a -1e30 plateau, signed zeros
    bb = np.concatenate([np.full(50, -np.inf), np.full(80, -1e30), np.full(120, -np.inf), [-0.0, 0.0, 0.0, -1e30]])
    runs.append((ll, bb))
    logl, birth, _ = simulate(80, 4, 100, 39)                                 # off-contour rows, rows shuffled
    pick = rng.choice(np.flatnonzero(birth > -np.inf), 12, replace=False)
    logl[pick[:6]] = birth[pick[:6]]
    logl[pick[6:]] = birth[pick[6:]] - 1e-3
    perm = rng.permutation(len(logl))
    runs.append((logl[perm], birth[perm]))
    runs.append((np.array([2.0, 3.0, 1.0]), np.array([np.inf, 2.0, -np.inf])))
    return runs


def _arrays(runs):
    logl = np.concatenate([r[0] for r in runs])
    birth = np.concatenate([r[1] for r in runs])
    return logl, birth, np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int64)


def test_device_indexes_are_the_definition(gpu_required):
    runs = _ragged_runs()
    logl, birth, rs = _arrays(runs)
    ref = insertion.indexes_arrays(logl, birth, rs)
    timing = {}
    got = insertion.indexes_arrays(logl, birth, rs, device=0, timing=timing)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert timing["rows"] == len(logl) and timing["launches"] == 4 and timing["kernel_ms"] > 0
    again = insertion.indexes_arrays(logl, birth, rs, device=0)
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    for r, (ll, bb) in enumerate(runs):                                      # each run alone gives its rows of the batch
        i1, n1 = insertion.indexes_arrays(ll, bb, [0, len(ll)], device=0)
        assert np.array_equal(i1, got[0][rs[r]:rs[r + 1]]) and np.array_equal(n1, got[1][rs[r]:rs[r + 1]]), r


def test_128_runs_in_one_call(gpu_required):
    runs = [simulate(100, 25 if r % 2 else 1, 40 if r % 2 else 1000, 100 + r)[:2] for r in range(128)]
    logl, birth, rs = _arrays(runs)
    got = insertion.indexes_arrays(logl, birth, rs, device=0)
    sub = [0, 1, 64, 127]                                                    # the definition on a few of them
    ref = insertion.indexes_arrays(*_arrays([runs[r] for r in sub]))
    mine = np.concatenate([got[0][rs[r]:rs[r + 1]] for r in sub]), np.concatenate([got[1][rs[r]:rs[r + 1]] for r in sub])
    assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
    ins = birth > -np.inf
    assert np.all(got[1][ins] == 100)


def test_refusals(gpu_required):
    lib = _abi.load()
    logl, birth = np.array([1.0, 2.0, 3.0]), np.array([-np.inf, 1.0, 2.0])
    out_i, out_n = np.empty(3, dtype=np.int32), np.empty(3, dtype=np.int32)

    def call(ll, bb, rs, n_rows=None, n_runs=None):
        rs = np.asarray(rs, dtype=np.int64)
        return lib.rvll_insertion_indexes(0, _abi.as_dp(ll), _abi.as_dp(bb), len(ll) if n_rows is None else n_rows,
                                          rs.ctypes.data_as(C.POINTER(C.c_int64)), len(rs) - 1 if n_runs is None else n_runs,
                                          _abi.as_ip(out_i), _abi.as_ip(out_n), None)

    assert call(logl, birth, [0, 3]) == _abi.OK
    assert call(np.array([1.0, np.nan, 3.0]), birth, [0, 3]) == _abi.E_INVALID
    assert call(logl, np.array([-np.inf, np.nan, 2.0]), [0, 3]) == _abi.E_INVALID
    assert call(logl, birth, [0, 2]) == _abi.E_INVALID                        # does not reach n_rows
    assert call(logl, birth, [1, 3]) == _abi.E_INVALID                        # does not start at 0
    assert call(logl, birth, [0, 3, 2, 3]) == _abi.E_INVALID                  # falls
    assert call(logl, birth, [0, 3], n_runs=0) == _abi.E_INVALID
    assert call(logl, birth, [0, 2 ** 31], n_rows=2 ** 31) == _abi.E_INVALID  # a run of 2^31 rows (refused before any read)
    with pytest.raises(ValueError):
        insertion.indexes_arrays([1.0, np.nan], [-np.inf, 0.0], [0, 2], device=0)


def _check_births(res, nlive, kbatch):
    """The invariants of a correct sampler's births; returns the off-contour rows (the exact redo of a wandering solve)."""
    birth, logl = res.logl_birth, res.logl
    assert birth is not None and birth.shape == logl.shape
    tops = logl[kbatch - 1:res.niter:kbatch]
    fin = birth > -np.inf
    assert np.count_nonzero(~fin) == nlive
    assert np.all(np.isin(birth[fin], tops))
    offc = fin & (logl <= birth)
    index, n_at = insertion.indexes([res], device=0)[0]
    ref_i, ref_n = insertion.indexes([res])[0]                              # the numpy definition
    assert np.array_equal(index, ref_i) and np.array_equal(n_at, ref_n)
    assert np.all(n_at[fin & ~offc] == nlive)
    return int(np.count_nonzero(offc))


def test_resident_ensemble_births_are_the_standalone_runs(gpu_required):
    seeds = (1, 2, 3)
    with _51peg() as m:
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=8_000_000)
        ens = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        cl = run_nested_ensemble(None, None, m.ndim, seeds, live=m, clustering=True, **kw)
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw) for s in seeds]
        alone_cl = [run_nested_slice(None, None, m.ndim, seed=s, live=m, clustering=True, **kw) for s in seeds]
    for s, e, c, a, ac in zip(seeds, ens, cl, alone, alone_cl):
        assert np.array_equal(e.logl, a.logl) and np.array_equal(e.logl_birth, a.logl_birth), s
        assert np.array_equal(c.logl, ac.logl) and np.array_equal(c.logl_birth, ac.logl_birth), s
        off = [_check_births(r, 400, 100) for r in (e, c)]
        assert off == [0, 0], (s, off)
    out = insertion.test(ens + cl, device=0)
    assert out["pooled"]["off_contour"] == 0
    assert all(rec == ref for rec, ref in zip(_plain(out["runs"]), _plain(insertion.test(ens + cl)["runs"])))


def _plain(recs):
    return [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in rec.items()} for rec in recs]


def test_host_chol_births_are_the_host_managed_walk(gpu_required):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=2000, kbatch=500, nsteps=9, dlogz=1e-9, max_calls=300_000, wrapped=wrapped_params(m.parnames), seed=4)
        ref = run_nested_slice(prior, loglike, m.ndim, walker=m.slice_walk, **kw)
        got = run_nested_slice(None, None, m.ndim, live=m, live_chol="host", **kw)
        dead_b, live_b = m.live_births()
    assert got.niter == ref.niter and np.array_equal(got.logl, ref.logl)
    assert np.array_equal(got.logl_birth, ref.logl_birth)
    assert np.array_equal(np.concatenate([dead_b, live_b]), got.logl_birth)
    assert _check_births(got, 2000, 500) == 0


def test_refused_steps_leave_the_births_as_they_were(gpu_required):
    R, n, kdead = 3, 200, 50
    rng = np.random.default_rng(4)
    runs = np.arange(R, dtype=np.int32)

    def births(m):
        return [m.live_runs_births(r) for r in range(R)]

    def same(a, b):
        return all(np.array_equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))

    with _gaussian() as m:
        m.live_runs_init(rng.random((R * n, 2)), R)
        b0 = births(m)
        assert all(len(d) == 0 and np.all(lv == -np.inf) and len(lv) == n for d, lv in b0)
        dl, lstar, _ = m.live_runs_sort(runs, kdead)
        ranks = rng.integers(0, n - kdead, (R, kdead))
        m.live_runs_step(runs, kdead, ranks, lstar, None, 4, 200, [1, 2, 3])
        before = births(m)
        for r in range(R):
            dead, lv = before[r]
            assert len(dead) == kdead and np.all(dead == -np.inf)
            assert np.count_nonzero(lv == lstar[r]) == kdead and np.count_nonzero(lv == -np.inf) == n - kdead
        with pytest.raises(RvllError):                                     # no sort since the last step
            m.live_runs_step(runs, kdead, ranks, lstar, None, 4, 200, [1, 2, 3])
        assert same(births(m), before)
        dl, lstar2, _ = m.live_runs_sort(runs, kdead)
        bad = ranks.copy()
        bad[1, 7] = n - kdead
        with pytest.raises(RvllError):                                     # a rank outside the survivors
            m.live_runs_step(runs, kdead, bad, lstar2, None, 4, 200, [1, 2, 3])
        with pytest.raises(RvllError):                                     # an lstar that is not the sort's
            m.live_runs_step(runs, kdead, ranks, lstar2 + 1.0, None, 4, 200, [1, 2, 3])
        with pytest.raises(RvllError):                                     # an nboot out of range, in the clustered step
            m.live_runs_step_clustered(runs, kdead, ranks, lstar2, None, 4, 200, [1, 2, 3], 99, [5, 6, 7])
        assert same(births(m), before)
        # the one-run call refuses the ensemble, and the ensemble's refuses a run out of range
        cnt = C.c_int64(0)
        assert _abi.load().rvll_live_births(m._h, C.byref(cnt), None, None) == _abi.E_INVALID
        assert _abi.load().rvll_live_runs_births(m._h, R, C.byref(cnt), None, None) == _abi.E_INVALID
        dl, lstar3, _ = m.live_runs_sort(runs, kdead)
        m.live_runs_step(runs, kdead, ranks, lstar3, None, 4, 200, [1, 2, 3])
        after = births(m)
        for r in range(R):
            assert np.array_equal(after[r][0][:kdead], before[r][0])
            assert np.count_nonzero(after[r][0] == lstar[r]) + np.count_nonzero(after[r][1] == lstar[r]) == kdead
        # and the one-run set: its births start at -inf, the ensemble's call refuses it
        m.live_init(rng.random((n, 2)))
        d1, l1 = m.live_births()
        assert len(d1) == 0 and np.all(l1 == -np.inf)
        assert _abi.load().rvll_live_runs_births(m._h, 0, C.byref(cnt), None, None) == _abi.E_INVALID
