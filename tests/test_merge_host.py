"""CPU: merging runs by their birth contours (evidence_amd/merge.py).  One run merged alone dies by its own (nlive, kbatch)
schedule and then at m, m - 1, ..., 1; the definition matches a per-row brute force on ragged runs with ties across runs, a
-1e30 plateau and off-contour rows, with and without run multiplicities; the merged evidence of a Gaussian toy is right within
its bootstrap error, which is about 1/sqrt(R) of one run's; malformed inputs are refused."""
import math

import numpy as np
import pytest

from evidence_amd import merge, shrinkage
from evidence_amd.nested import NestedResult, run_nested, run_nested_slice


def prior(cube):
    return -10.0 + 20.0 * cube


def loglike(x):
    return -0.5 * np.sum(x * x, axis=1)


TRUTH = math.log(2.0 * math.pi / 400.0)       # the Gaussian's mass over the uniform prior box of side 20


def _result(logl, birth):
    logl = np.asarray(logl, dtype=np.float64)
    return NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=None, logl=logl,
                        logwt=np.zeros_like(logl), logl_birth=np.asarray(birth, dtype=np.float64))


def _synthetic(rng, nlive, n_dead, kbatch=1, plateau=0, off=0, tie_grid=None):
    """One run made as a sampler makes it: nlive points from -inf, kbatch deaths an iteration, each replacement born on the
    iteration's highest dead log-L and drawn above it; optionally a -1e30 plateau at the start, log-L rounded to a grid (ties
    across runs) and `off` rows lowered onto or below their birth."""
    live = list(rng.normal(-30.0, 5.0, nlive))
    if plateau:
        live[:plateau] = [-1e30] * plateau
    births = [-np.inf] * nlive
    rows_l, rows_b = [], []
    for _ in range(n_dead // kbatch):
        idx = np.argsort(live, kind="stable")[:kbatch]
        lstar = max(live[j] for j in idx)
        for j in idx:
            rows_l.append(live[j])
            rows_b.append(births[j])
            base = lstar if lstar > -1e29 else -60.0                     # the first draws off the plateau
            new = base + rng.exponential(3.0)
            if tie_grid:
                new = base + tie_grid * max(1, round((new - base) / tie_grid))
            live[j], births[j] = new, lstar
    logl = np.array(rows_l + live)
    birth = np.array(rows_b + births)
    if off:
        cand = np.flatnonzero(birth > -np.inf)
        pick = rng.choice(cand, off, replace=False)
        logl[pick[: off // 2]] = birth[pick[: off // 2]]                # on the contour
        logl[pick[off // 2:]] = birth[pick[off // 2:]] - 0.25           # below it
    perm = rng.permutation(logl.shape[0])                                # any order inside a run
    return logl[perm], birth[perm]


def _ragged(seed=0):
    rng = np.random.default_rng(seed)
    return [_synthetic(rng, 12, 60, kbatch=3, plateau=4, tie_grid=0.5),
            _synthetic(rng, 5, 7, tie_grid=0.5, off=2),
            _synthetic(rng, 30, 400, kbatch=10, off=5, tie_grid=0.5),
            _synthetic(rng, 1, 0),
            _synthetic(rng, 8, 24, kbatch=2, plateau=2, off=3)]


def _arrays(runs):
    logl = np.concatenate([r[0] for r in runs])
    birth = np.concatenate([r[1] for r in runs])
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int64)
    return logl, birth, run_start


def _brute(runs, w=None, seed=None):
    """Row by row, in plain Python floats: (order, n, logz, information, logw) with multiplicities w (1 each by default);
    seed=None: expected shrinkage, else the random draws of replicate 0 with that seed."""
    w = [1] * len(runs) if w is None else list(w)
    rows = [(float(l), r, p, float(b)) for r, (ll, bb) in enumerate(runs) for p, (l, b) in enumerate(zip(ll, bb))]
    keyed = sorted(range(len(rows)), key=lambda g: (rows[g][0], rows[g][1], rows[g][2]))
    beff = [np.nextafter(l, -np.inf) if l <= b else b for (l, _, _, b) in rows]
    logx, died, out_n, logw = 0.0, 0, [], []
    for i, g in enumerate(keyed):
        L, r = rows[g][0], rows[g][1]
        n = sum(w[rows[k][1]] for k in range(len(rows)) if beff[k] < L) - sum(w[rows[keyed[j]][1]] for j in range(i))
        out_n.append(n)
        delta = 0.0
        for q in range(w[r]):
            if seed is None:
                delta += -1.0 / (n - q)
            else:
                u = 1.0 - float(merge.uniform_at(np.uint64(seed), np.uint64(died + q)))
                delta += math.log(u) / (n - q)
        logw.append((L + logx) + math.log(-math.expm1(delta)) if w[r] else -math.inf)
        logx += delta
        died += w[r]
    top = max(logw)
    s = sum(math.exp(x - top) for x in logw if x > -math.inf)
    lnz = top + math.log(s)
    h = sum(math.exp(x - lnz) * rows[g][0] for x, g in zip(logw, keyed) if x > -math.inf) - lnz
    return np.array(keyed), np.array(out_n), lnz, h, np.array(logw)


def test_one_run_dies_by_its_own_schedule_then_m_down_to_one():
    res = run_nested_slice(prior, loglike, 2, nlive=100, kbatch=7, nsteps=4, seed=7, max_calls=60_000)
    assert res.kbatch == 7 and res.niter % 7 == 0 and res.logl_birth is not None
    assert np.unique(res.logl).size == res.logl.size                    # a smooth toy: no tied log-L
    got = merge.merge([res])
    nd, m = res.niter, len(res.logl) - res.niter
    assert np.array_equal(got.nlive_row[:nd], shrinkage.live_counts(nd, 100, 7))
    assert np.array_equal(got.nlive_row[nd:], np.arange(m, 0, -1))
    assert np.array_equal(got.logl, np.sort(res.logl)) and np.all(got.run_index == 0)
    assert got.nlive is None and got.kbatch is None and got.niter == len(res.logl)
    sd = shrinkage.logz_error([res], nsamples=300, seed=3)[0]
    assert abs(got.logz - res.logz) < sd, (got.logz, res.logz, sd)
    assert np.isclose(np.logaddexp.reduce(got.logwt), 0.0, atol=1e-12)
    assert got.logzerr == pytest.approx(math.sqrt(got.information / got.nlive_row[0]))
    assert got.samples.shape == res.samples.shape
    assert np.array_equal(got.samples, res.samples[np.argsort(res.logl, kind="stable")])


def test_the_definition_matches_a_brute_force_row_loop():
    runs = _ragged()
    logl, birth, run_start = _arrays(runs)
    got = merge.merge_arrays(logl, birth, run_start)
    order, n, lnz, h, logw = _brute(runs)
    assert np.array_equal(got["order"], order)
    assert np.array_equal(got["nlive_row"], n) and n.min() >= 1
    assert got["off_contour"] == 10
    assert abs(got["logz"] - lnz) <= 1e-12 * abs(lnz)
    assert abs(got["information"] - h) <= 1e-12 * max(1.0, abs(h))
    fin = logw > -1e29
    assert np.allclose(got["logwt"][fin], (logw - lnz)[fin], rtol=0, atol=1e-11)
    assert np.allclose(got["logwt"][~fin], (logw - lnz)[~fin], rtol=1e-15, atol=0)
    assert np.array_equal(got["run_index"], np.repeat(np.arange(5), np.diff(run_start))[order])
    # ties across runs exist, and the -1e30 plateau is merged
    ll = logl[order]
    assert np.any((ll[1:] == ll[:-1]) & (got["run_index"][1:] != got["run_index"][:-1]))
    assert np.count_nonzero(ll == -1e30) == 6


@pytest.mark.parametrize("s", [0, 1, 5])
def test_random_and_bootstrap_replicates_match_the_brute_force(s):
    runs = _ragged(1)
    logl, birth, run_start = _arrays(runs)
    seed = 1234
    logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, nsamples=s + 1, seed=seed, mode="random",
                                                bootstrap=True, return_logwt=True)
    seed_s = int(shrinkage.replicate_seeds(seed, s + 1)[s])
    w = merge.bootstrap_weights([seed_s], len(runs))[0]
    assert w.sum() == len(runs)
    _, _, lnz, h, logw = _brute(runs, w=w, seed=seed_s)
    assert abs(logz[s] - lnz) <= 1e-12 * abs(lnz)
    assert abs(info[s] - h) <= 1e-11 * max(1.0, abs(h))
    fin = logw > -1e29
    assert np.allclose(logwt[s][fin], (logw - lnz)[fin], rtol=0, atol=1e-11)
    assert np.all(np.isneginf(logwt[s][np.isneginf(logw)]))


def test_bootstrap_weights_repeat_and_drop_runs():
    w = merge.bootstrap_weights(shrinkage.replicate_seeds(9, 200), 16)
    assert np.all(w.sum(axis=1) == 16)
    assert (w == 0).any() and (w >= 2).any()
    assert abs(w.mean() - 1.0) < 1e-12


def test_the_order_of_the_runs_does_not_matter():
    a, b, c = _ragged(2)[:3]
    ab = merge.merge([_result(*a), _result(*b), _result(*c)])
    ba = merge.merge([_result(*c), _result(*b), _result(*a)])
    assert ab.logz == ba.logz and ab.information == ba.information
    assert np.array_equal(ab.nlive_row, ba.nlive_row) and np.array_equal(ab.logl, ba.logl)


def test_expected_replicates_without_the_bootstrap_are_the_merge():
    logl, birth, run_start = _arrays(_ragged(3))
    one = merge.merge_arrays(logl, birth, run_start)
    logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, nsamples=5, mode="expected", bootstrap=False,
                                                return_logwt=True)
    assert np.all(logz == one["logz"]) and np.all(info == one["information"])
    assert all(np.array_equal(row, one["logwt"]) for row in logwt)


def test_merged_gaussian_evidence_is_right_within_its_error():
    runs = [run_nested(prior, loglike, 2, nlive=100, dlogz=0.01, seed=40 + k) for k in range(8)]
    merged = merge.merge(runs)
    assert merged.nlive_row[0] == 800 and merged.niter == sum(len(r.logl) for r in runs)
    boot = merge.logz_error(runs, nsamples=300, seed=5)
    shrink = merge.logz_error(runs, nsamples=300, seed=5, bootstrap=False)
    single = merge.logz_error(runs[:1], nsamples=300, seed=5, bootstrap=False)
    assert abs(merged.logz - TRUTH) < 4 * max(boot, shrink), (merged.logz, TRUTH, boot, shrink)
    assert 0.25 * single < shrink < 0.75 * single, (shrink, single)
    assert abs(merged.logz - TRUTH) < 4 * single


@pytest.mark.parametrize("n_runs", [24, 96])
@pytest.mark.parametrize("mode, bootstrap", [("expected", False), ("random", True)])
def test_the_wide_fixture_spreads_its_mass_over_the_merged_order(mode, bootstrap, n_runs):
    """The device tests that weigh every row (the _wide tests of tests/test_gpu_*.py) rest on this: in the definition's 62-bit
    fixed-point weights of _wide, at least 95 % of the 1024-row tiles of the merged order hold 0.1 / ntiles of the mass or more,
    and no tile of the 2 112 000-row default (2063 tiles) holds over 1 %.  Conditions on the fixture, not measurements: the
    worst of the replicates here has 2058 of 2063 tiles above the floor and a largest tile of 0.29 %.

    A tile's share goes as 1 / ntiles, so the ceiling is 1 % · 2063 / ntiles: 20.6 mean tiles at either size.  At 24 runs
    (528 000 rows, 516 tiles: the draws' fixture) 515 tiles are above the floor and the largest holds 1.02 - 1.04 %, 5.3 - 5.4 mean
    tiles (5.6 - 5.9 at 96 runs); a flat 1 % is 5.2 mean tiles there and does not hold."""
    from evidence_amd import draws
    from test_gpu_merge import _wide
    logl, birth, run_start = _wide(n_runs=n_runs)
    assert logl.size == n_runs * 22_000
    _, _, logwt = merge.replicates_arrays(logl, birth, run_start, nsamples=2, seed=3, mode=mode, bootstrap=bootstrap,
                                          return_logwt=True)
    ntiles = -(-logl.size // 1024)
    for s in range(2):
        m = draws.fixed_point(logwt[s])
        share = np.add.reduceat(m, np.arange(0, m.size, 1024)).astype(np.float64) / float(m.sum(dtype=np.int64))
        assert share.size == ntiles
        print(mode, bootstrap, s, "rows with mass", int(np.count_nonzero(m)), "of", m.size, " tiles above the floor",
              int(np.count_nonzero(share >= 0.1 / ntiles)), "of", ntiles, " largest tile", float(share.max()))
        assert np.count_nonzero(share >= 0.1 / ntiles) >= 0.95 * ntiles
        assert share.max() <= 0.01 * 2063 / ntiles


def test_refusals():
    logl, birth, run_start = _arrays(_ragged(4))
    with pytest.raises(ValueError, match="birth"):
        merge.merge([_result(logl[:5], birth[:5]), NestedResult(0.0, 0.0, 0, 0, 0.0, None, logl[5:9], logl[5:9])])
    bad = logl.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        merge.merge_arrays(bad, birth, run_start)
    bad[3] = -np.inf
    with pytest.raises(ValueError, match="finite"):
        merge.replicates_arrays(bad, birth, run_start, nsamples=2)
    nanb = birth.copy()
    nanb[0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        merge.merge_arrays(logl, nanb, run_start)
    for rs in (run_start[:-1], np.r_[1, run_start[1:]], np.r_[run_start[:-1], run_start[-1] + 1], run_start[::-1]):
        with pytest.raises(ValueError, match="run_start"):
            merge.merge_arrays(logl, birth, rs)
    with pytest.raises(ValueError, match="mode"):
        merge.replicates_arrays(logl, birth, run_start, mode="mean")
    with pytest.raises(ValueError, match="nsamples"):
        merge.replicates_arrays(logl, birth, run_start, nsamples=0)
    with pytest.raises(ValueError):
        merge.merge([])
