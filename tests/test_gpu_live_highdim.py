"""The resident live set's moments, order and wide-row moves at the dimensions and row counts where their kernels change path
(csrc/rvll_live.hip; cases and references: tests/highdim_cases.py).

The factor.  live_step(..., return_chol=True) returns the lower factor of the survivors' covariance, summed on the device
(moments_sum / moments_cov: 128 block partials, folded in quarters) and factored on the host (whitening_factor).  It is compared
with the longdouble factor of the downloaded survivors within FACTOR_MARGIN = 64 times the distance of the float64 numpy factor
from that reference, per case (a few 1e-14 of max|L|; test_highdim_cases_host.py prints the distances), never looser than 1e-12.
The errors this is for — a (j, l) pair summed into the wrong word, a row group summed twice or not at all, a second staging
round that starts from zero — are of order 1e-3 and more.

The order.  rvll_live_sort and the segmented sort of the ensemble against numpy's stable argsort on log-L of both signs (both
branches of the sort key) with exact ties (40 duplicated rows): ties go by row.
"""
import numpy as np
import pytest

import highdim_cases as hc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def _factor_step(m, cube, kdead, wrapped, seed=5):
    """live_init + one live_step of one move with the device's own factor: (order, rows before, rows after, new log-L, factor)."""
    logl = m.live_init(cube)
    order = np.argsort(logl, kind="stable").astype(np.int32)
    before = m.live_get()
    assert np.array_equal(before[0], cube) and np.array_equal(before[2], logl)
    start = order[kdead:][np.random.default_rng(seed).integers(0, len(cube) - kdead, kdead)]
    new_l, used, chol = m.live_step(order, kdead, start, float(logl[order[kdead - 1]]), wrapped, nsteps=1, seed=seed, return_chol=True)
    return order, before, m.live_get(), new_l, chol


@pytest.mark.parametrize("ndim, nsurv", hc.FACTOR_CASES)
def test_the_factor_of_the_survivors(gpu_required, ndim, nsurv):
    """(7, 32): 96 of the 128 blocks get no row; (45, 400) | (46, 400): the (j, l) sums in registers | in global memory;
    (64, 129): one block with two rows; (64, 4097), (129, 4097): a second staging round of moments_cov; (128, 300) | (129, 300):
    two row groups a block | one in moments_sum."""
    kdead = hc.FACTOR_KDEAD
    with hc.offsets_model(ndim) as m:
        order, before, after, new_l, chol = _factor_step(m, hc.live_cube(ndim, nsurv), kdead, hc.wrapped(ndim))
    rows = before[0][order[kdead:]]
    assert rows.shape == (nsurv, ndim)
    bound, host, ref = hc.factor_bound(rows)
    dist = hc.factor_distance(chol, ref)
    print(f"live factor D {ndim:3d} n {nsurv:4d}: device - longdouble {dist:.2e} of max|L|, bound {bound:.2e} (float64 numpy {host:.2e})")
    assert np.all(np.triu(chol, 1) == 0) and np.all(np.diag(chol) > 0)
    assert dist <= bound
    assert np.array_equal(after[0][order[kdead:]], rows) and np.array_equal(after[2][order[:kdead]], new_l)


def test_ensemble_factors_at_46_parameters_are_each_runs_own(gpu_required):
    """live_runs_step(..., return_chol=True) on three of four runs at D = 46 (moments_cov's global-memory sums, a set a
    blockIdx.y): every run's factor is bit for bit its own live_step factor, as test_gpu_resident_ensemble.py asserts at D = 7,
    and meets the bound."""
    ndim, R, n, kdead = 46, 4, 200, 20
    runs = np.array([0, 2, 3], dtype=np.int32)
    rng = np.random.default_rng(46)
    wrapped = hc.wrapped(ndim)
    with hc.offsets_model(ndim) as m:
        cube = rng.random((R * n, ndim))
        m.live_runs_init(cube, R)
        dl, lstar, top = m.live_runs_sort(runs, kdead)
        ranks = rng.integers(0, n - kdead, (runs.size, kdead))
        seeds = [int(v) for v in rng.integers(0, 2 ** 62, runs.size)]
        wl, used, chols = m.live_runs_step(runs, kdead, ranks, lstar, wrapped, 2, 200, seeds, return_chol=True)
        for a, r in enumerate(runs):
            own = cube[r * n:(r + 1) * n]
            logl = m.live_init(own)
            order = np.argsort(logl, kind="stable")
            dl1, lstar1, top1 = m.live_sort(kdead)
            assert np.array_equal(dl[a], dl1) and lstar[a] == lstar1 and top[a] == top1
            wl1, used1, chol1 = m.live_step(None, kdead, ranks[a], lstar1, wrapped, 2, 200, seeds[a], return_chol=True)
            assert np.array_equal(chols[a], chol1) and np.array_equal(wl[a], wl1) and used[a] == used1, r
            bound, host, ref = hc.factor_bound(own[order[kdead:]])
            dist = hc.factor_distance(chols[a], ref)
            print(f"ensemble factor D {ndim} run {r}: device - longdouble {dist:.2e} of max|L|, bound {bound:.2e}")
            assert dist <= bound and np.all(np.triu(chols[a], 1) == 0)


def _replaced(before, after):
    return np.flatnonzero(np.any(before[0] != after[0], axis=1) | (before[2] != after[2]))


def test_live_sort_is_the_stable_order_with_ties_and_both_signs(gpu_required):
    n, ndup, kdead = 400, 40, 120
    with hc.offsets_model(hc.SORT_NDIM, hc.SORT_SVRAD) as m:
        cube = hc.sort_cube(n, ndup, 31)
        logl = m.live_init(cube)
        assert (logl > 0).sum() > 40 and (logl < 0).sum() > 40            # both branches of the sort key
        assert np.array_equal(logl[n - ndup:], m.prior_loglike_batch(cube[n - ndup:])[1]) and len(np.unique(logl)) <= n - ndup
        order = np.argsort(logl, kind="stable")
        tied_dead = np.flatnonzero(np.diff(logl[order[:kdead + 1]]) == 0)
        assert tied_dead.size >= 5                                         # ties among the dying rows and across the cut or not:
        dead, lstar, top = m.live_sort(kdead)
        assert np.array_equal(dead, logl[order[:kdead]]) and lstar == logl[order[kdead - 1]] and top == logl[order[-1]]
        before = m.live_get()
        ranks = np.random.default_rng(2).integers(0, n - kdead, kdead)
        new_l, used = m.live_step(None, kdead, ranks, lstar, hc.wrapped(hc.SORT_NDIM), nsteps=3, seed=9)
        after = m.live_get()
        dth, dll = m.live_dead()
    # every walker moved (three moves inside a slice the start rows are inside of), so the rows that changed are the rows replaced
    assert np.array_equal(_replaced(before, after), np.sort(order[:kdead]))
    assert np.array_equal(after[2][order[:kdead]], new_l) and (new_l > lstar).all()
    assert np.array_equal(dll, logl[order[:kdead]]) and np.array_equal(dth, before[1][order[:kdead]])


def test_live_runs_sort_is_each_runs_stable_order_with_ties_inside_and_across_runs(gpu_required):
    R, n, kdead = 4, 200, 60
    runs = np.array([0, 1, 3], dtype=np.int32)
    with hc.offsets_model(hc.SORT_NDIM, hc.SORT_SVRAD) as m:
        cube = hc.sort_cube(R * n, 0, 32)
        rng = np.random.default_rng(33)
        cube[3 * n:3 * n + 15] = cube[0:15]                  # ties across runs: run 3 repeats rows of run 0 and of the unlisted run 2 ...
        cube[3 * n + 15:3 * n + 30] = cube[2 * n:2 * n + 15]
        for r in range(R):                                   # ... and inside every run: its last 20 rows repeat earlier ones
            own = cube[r * n:(r + 1) * n]
            own[n - 20:] = own[rng.choice(n - 20, 20, replace=False)]
        logl = m.live_runs_init(cube, R)
        assert (logl > 0).sum() > 40 and (logl < 0).sum() > 40
        assert np.array_equal(logl[3, :15], logl[0, :15]) and all(len(np.unique(logl[r])) <= n - 20 for r in range(R))
        orders = [np.argsort(logl[r], kind="stable") for r in range(R)]
        dead, lstar, top = m.live_runs_sort(runs, kdead)
        for a, r in enumerate(runs):
            assert np.array_equal(dead[a], logl[r][orders[r][:kdead]]) and lstar[a] == logl[r][orders[r][kdead - 1]], r
            assert top[a] == logl[r][orders[r][-1]], r
        before = [m.live_runs_get(r) for r in range(R)]
        ranks = rng.integers(0, n - kdead, (runs.size, kdead))
        new_l, used = m.live_runs_step(runs, kdead, ranks, lstar, hc.wrapped(hc.SORT_NDIM), 3, 200, [11, 12, 13])
        after = [m.live_runs_get(r) for r in range(R)]
        deads = [m.live_runs_dead(r) for r in range(R)]
    for r in range(R):
        if r not in runs:
            assert _replaced(before[r], after[r]).size == 0 and len(deads[r][1]) == 0
            continue
        a = int(np.flatnonzero(runs == r)[0])
        assert np.array_equal(_replaced(before[r], after[r]), np.sort(orders[r][:kdead])), r
        assert np.array_equal(after[r][2][orders[r][:kdead]], new_l[a]) and (new_l[a] > lstar[a]).all()
        assert np.array_equal(deads[r][1], logl[r][orders[r][:kdead]]) and np.array_equal(deads[r][0], before[r][1][orders[r][:kdead]])


def test_wide_rows_move_whole_at_129_parameters(gpu_required):
    """The gathers and scatters of a step with rows of 129 doubles: the survivors bit-identical, the new rows at order[:kdead]
    (each the prior transform and log-L of its own cube row), the dead store holding the old rows' theta and log-L in order —
    over two steps, the second from walked rows."""
    ndim, n, kdead = 129, 300, 37
    wrapped = hc.wrapped(ndim)
    rng = np.random.default_rng(129)
    with hc.offsets_model(ndim) as m:
        cube = rng.random((n, ndim))
        logl = m.live_init(cube)
        dead_t, dead_l = [], []
        for it in range(2):
            u0, t0, l0 = m.live_get()
            order = np.argsort(l0, kind="stable").astype(np.int32)
            start = order[kdead:][rng.integers(0, n - kdead, kdead)]
            new_l, used = m.live_step(order, kdead, start, float(l0[order[kdead - 1]]), wrapped, nsteps=3, seed=40 + it)
            u1, t1, l1 = m.live_get()
            rest, gone = order[kdead:], order[:kdead]
            assert np.array_equal(u1[rest], u0[rest]) and np.array_equal(t1[rest], t0[rest]) and np.array_equal(l1[rest], l0[rest])
            assert np.array_equal(l1[gone], new_l) and (new_l > l0[order[kdead - 1]]).all()
            assert np.all(np.any(u1[gone] != u0[gone], axis=1)) and np.array_equal(_replaced((u0, t0, l0), (u1, t1, l1)), np.sort(gone))
            th, ll = m.prior_loglike_batch(u1[gone])
            assert np.array_equal(th, t1[gone]) and np.array_equal(ll, l1[gone])
            dead_t.append(t0[gone])
            dead_l.append(l0[gone])
            dth, dll = m.live_dead()
            assert np.array_equal(dth, np.concatenate(dead_t)) and np.array_equal(dll, np.concatenate(dead_l))
        assert np.array_equal(logl, m.prior_loglike_batch(cube)[1])
