"""CPU: equal-weight draws of merged runs (evidence_amd/draws.py).  The numpy definition on the ragged runs of the merge tests and
on the 3212 rows of the marginal tests, for both shrinkage modes with and without the run bootstrap and 1, 64 and 1000 draws: every
row is drawn floor or ceil of n p times, a row without weight never, the draws ascend in merged order, a replicate alone equals
itself among 64, a replicate of empty runs is -1 throughout; a brute-force loop in Python integers on 40 rows; refusals; the library
exports the entry."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import _abi, draws, merge
from evidence_amd.shrinkage import replicate_seeds
from test_marginals_host import _small, _with_empty_runs
from test_merge_host import _arrays, _ragged, _synthetic

S = 64
CASES = {"ragged0": lambda: _arrays(_ragged(0)), "ragged1": lambda: _arrays(_ragged(1)), "ragged2": lambda: _arrays(_ragged(2)),
         "small": _small}
_WEIGHTS = {}


def _weights(case, mode, bootstrap):
    """(arrays, merged order, m [S, N] int64, logz) of the case by merge.replicates_arrays: computed once, shared, never changed."""
    key = (case, mode, bootstrap)
    if key not in _WEIGHTS:
        logl, birth, run_start = CASES[case]()
        logz, _, logwt = merge.replicates_arrays(logl, birth, run_start, S, seed=5, mode=mode, bootstrap=bootstrap, return_logwt=True)
        m = draws.fixed_point(logwt)
        order = merge._layout(logl, birth, run_start)["order"].astype(np.int64)
        for v in (m, order, logz):
            v.setflags(write=False)
        _WEIGHTS[key] = ((logl, birth, run_start), order, m, logz)
    return _WEIGHTS[key]


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
@pytest.mark.parametrize("case", list(CASES))
def test_counts_zero_rows_and_order(case, mode, bootstrap):
    arrays, order, m, logz = _weights(case, mode, bootstrap)
    N = order.size
    merged_pos = np.empty(N, np.int64)
    merged_pos[order] = np.arange(N)
    for n in (1, 64, 1000):
        rows, lz, _ = draws.draw_arrays(*arrays, n, S, seed=5, mode=mode, bootstrap=bootstrap)
        assert rows.shape == (S, n) and rows.dtype == np.int64 and np.array_equal(lz, logz)
        assert rows.min() >= 0 and rows.max() < N
        pos = merged_pos[rows]
        assert np.all(np.diff(pos, axis=1) >= 0)                          # ascending in merged order
        for s in range(S):
            M = int(m[s].sum())
            cnt = np.bincount(pos[s], minlength=N)
            lo = np.array([int(n) * int(v) // M for v in m[s]])           # floor(n p), p = m / M exactly, in Python integers
            exact = np.array([(int(n) * int(v)) % M == 0 for v in m[s]])
            assert np.all((cnt == lo) | ((cnt == lo + 1) & ~exact)), (n, s)
            assert np.all(cnt[m[s] == 0] == 0)
        alone = draws.draw_arrays(*arrays, n, 1, seed=int(replicate_seeds(5, S)[S - 1]), mode=mode, bootstrap=bootstrap)[0]
        assert np.array_equal(alone[0], rows[S - 1])                      # replicate s alone: its seed is all it has


def test_expected_replicates_without_the_bootstrap_differ_by_their_uniform_only():
    arrays, order, m, _ = _weights("small", "expected", False)
    assert np.all(m == m[0])
    rows, _, _ = draws.draw_arrays(*arrays, 64, S, seed=5, mode="expected", bootstrap=False)
    seeds = replicate_seeds(5, S)
    for s in range(S):
        assert np.array_equal(rows[s], order[draws.pick(m[0], seeds[s], 64)])
    assert len({tuple(r) for r in rows}) > 1                              # and the uniforms do differ
    one = draws.draw_arrays(*arrays, 64, 1, seed=5, mode="expected", bootstrap=False)[0]
    assert np.array_equal(one[0], rows[0])                                # the plain equal-weight sample of the merged run


def test_a_replicate_of_empty_runs_is_minus_one_throughout():
    logl, birth, run_start, seed = _with_empty_runs()
    rows, logz, _ = draws.draw_arrays(logl, birth, run_start, 5, 12, seed=seed)
    dead = np.isneginf(logz)
    assert 0 < dead.sum() < 12
    assert np.all(rows[dead] == -1) and np.all(rows[~dead] >= 0)


def test_a_brute_force_loop_in_python_integers_agrees():
    rng = np.random.default_rng(3)
    runs = [_synthetic(rng, 6, 18, kbatch=2, tie_grid=0.5), _synthetic(rng, 4, 12, off=2)]
    logl, birth, run_start = _arrays(runs)
    assert logl.size == 40
    for mode, bootstrap in (("random", True), ("expected", False)):
        logz, _, logwt = merge.replicates_arrays(logl, birth, run_start, 7, seed=9, mode=mode, bootstrap=bootstrap, return_logwt=True)
        order = merge._layout(logl, birth, run_start)["order"]
        seeds = replicate_seeds(9, 7)
        for n in (1, 7, 64):
            rows, _, _ = draws.draw_arrays(logl, birth, run_start, n, 7, seed=9, mode=mode, bootstrap=bootstrap)
            for s in range(7):
                m = [int(round(float(np.exp(x)) * 2.0 ** 62)) if x > -np.inf else 0 for x in logwt[s]]
                M = sum(m)
                U = int(merge.uniform_at(np.uint64(int(seeds[s]) ^ draws.DRAW_XOR), 0) * 2.0 ** 53)
                assert U == draws.uniform53(int(seeds[s]) ^ draws.DRAW_XOR)
                Q = M // n
                O = (U * Q) >> 53
                want = []
                for k in range(n):
                    tau, run = k * Q + O, 0
                    for i in range(40):
                        run += m[i]
                        if run > tau:
                            want.append(int(order[i]))
                            break
                assert want == list(rows[s]), (mode, n, s)


def test_samples_stack_the_runs_as_merge_does():
    runs = _ragged(3)
    results = []
    for i, (l, b) in enumerate(runs):
        smp = np.stack([l, np.full(l.size, float(i))], axis=1)
        results.append(merge.NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=smp, logl=l,
                                    logwt=np.zeros_like(l), logl_birth=b))
    logl, birth, run_start = _arrays(runs)
    rows, logz, _ = draws.draw(results, 16, 3, seed=1)
    theta = draws.samples(results, 16, 3, seed=1)
    assert theta.shape == (3, 16, 2)
    assert np.array_equal(theta[..., 0], logl[rows])
    assert np.array_equal(theta[..., 1], (np.searchsorted(run_start, rows, side="right") - 1).astype(float))
    with pytest.raises(ValueError, match="samples"):
        draws.samples([merge.NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=None, logl=runs[0][0],
                                          logwt=np.zeros_like(runs[0][0]), logl_birth=runs[0][1])], 4, 2)


def test_refusals():
    logl, birth, run_start = _arrays(_ragged(4))
    for bad in (0, -1, 2 ** 20 + 1, 1.5):
        with pytest.raises(ValueError, match="ndraws"):
            draws.draw_arrays(logl, birth, run_start, bad, 2)
    draws.draw_arrays(logl, birth, run_start, 2 ** 20, 1)
    with pytest.raises(ValueError, match="nsamples"):
        draws.draw_arrays(logl, birth, run_start, 4, 0)
    with pytest.raises(ValueError, match="mode"):
        draws.draw_arrays(logl, birth, run_start, 4, 2, mode="mean")
    bad = logl.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        draws.draw_arrays(bad, birth, run_start, 4, 2)
    with pytest.raises(ValueError, match="run_start"):
        draws.draw_arrays(logl, birth, run_start[:-1], 4, 2)


def test_the_library_exports_the_entry_within_abi_0_8():
    assert "rvll_draw_replicates" in _abi.PROTOTYPES and _abi.ABI_VERSION == (0, 8)
    lib = _abi.load()
    assert hasattr(lib, "rvll_draw_replicates")
    assert C.sizeof(_abi.DrawTiming) == 7 * 8 + 3 * 8 + 4 * 4
