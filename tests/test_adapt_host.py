"""CPU: the step-count adaptation of the slice walk (adapt.py) — the distances, the rule, and the drivers with
adaptive_nsteps="move-distance": min == max == nsteps is the non-adaptive run bit for bit, the ensemble is the standalone runs
bit for bit, a correlated Gaussian started at one step lengthens its walks, and the Gaussian known answers still hold."""
import numpy as np
import pytest

from evidence_amd import adapt, run_nested_ensemble
from evidence_amd.nested import run_nested_slice


def prior(cube):
    return -10.0 + 20.0 * cube                                      # Uniform(-10, 10)


def loglike(x):
    return -0.5 * np.sum(x * x, axis=1)


LNZ_1D = float(np.log(np.sqrt(2 * np.pi) / 20.0))                  # -2.0768


# ---- the distances ----------------------------------------------------------------------------------------------------
def test_identity_factor_is_the_euclidean_distance():
    rng = np.random.default_rng(0)
    a, b = rng.random((50, 5)), rng.random((50, 5))
    got = adapt.dist(a, b, np.eye(5))
    assert np.allclose(got, np.linalg.norm(b - a, axis=1), rtol=1e-15, atol=0)


def test_scaled_and_sheared_factor_against_a_hand_solve():
    L = np.array([[2.0, 0.0], [1.0, 4.0]])
    a = np.array([[0.1, 0.2]])
    b = np.array([[0.5, 0.9]])
    # delta = (0.4, 0.7): z0 = 0.4 / 2 = 0.2, z1 = (0.7 - 1 * 0.2) / 4 = 0.125
    d0 = 0.5 - 0.1
    d1 = 0.9 - 0.2
    z0 = d0 / 2.0
    z1 = (d1 - (0.0 + 1.0 * z0)) / 4.0
    assert adapt.dist(a, b, L)[0] == np.sqrt(0.0 + z0 * z0 + z1 * z1)
    assert abs(adapt.dist(a, b, L)[0] - np.hypot(0.2, 0.125)) < 1e-15
    # the distance is symmetric and does not care about the sign of the step
    assert adapt.dist(b, a, L)[0] == adapt.dist(a, b, L)[0]


def test_wrapped_minimum_image_across_zero_and_one():
    a = np.array([[0.95, 0.95], [0.02, 0.5]])
    b = np.array([[0.05, 0.05], [0.98, 0.5]])
    plain = adapt.dist(a, b, np.eye(2))
    wrap = adapt.dist(a, b, np.eye(2), wrapped=[True, False])
    assert np.allclose(wrap, [np.hypot(0.1, 0.9), 0.04], atol=1e-15)
    assert np.allclose(plain, [np.hypot(0.9, 0.9), 0.96], atol=1e-15)
    both = adapt.dist(a, b, np.eye(2), wrapped=[True, True])
    assert np.allclose(both, [np.hypot(0.1, 0.1), 0.04], atol=1e-15)


def test_groups_of_size_zero_one_and_two():
    L = np.diag([0.5, 2.0])
    surv = np.array([[0.1, 0.1], [0.3, 0.5], [0.6, 0.6]])           # group 0: none, 1: row 0, 2: rows 1 and 2
    starts = np.array([[0.1, 0.1], [0.2, 0.2], [0.3, 0.5]])
    ends = np.array([[0.2, 0.3], [0.2, 0.2], [0.6, 0.6]])
    pair, move = adapt.walk_distances_runs(surv, [0, 0, 1, 3], np.stack([L, L, L]), None, starts, ends, [0, 1, 2])
    assert np.isnan(pair[0]) and np.isnan(pair[1])
    assert pair[2] == adapt.dist(surv[1:2], surv[2:3], L)[0]
    assert move[1] == 0.0
    assert move[2] == pair[2]
    counted, far = adapt.far_counts(pair, move, [0, 1, 2], [0, 0, 0], 1)
    assert counted[0] == 1 and far[0] == 0                          # equal is not far


def test_pair_mean_is_the_mean_over_unordered_pairs():
    rng = np.random.default_rng(3)
    rows = rng.random((9, 3))
    L = np.linalg.cholesky(np.cov(rows.T) + 1e-3 * np.eye(3))
    want = np.mean([adapt.dist(rows[i:i + 1], rows[j:j + 1], L)[0] for i in range(9) for j in range(i + 1, 9)])
    assert abs(adapt.pair_mean(rows, L) - want) <= 1e-14 * want


def test_refusals():
    with pytest.raises(ValueError):
        adapt.walk_distances_runs(np.zeros((2, 2)), [0, 3], np.eye(2)[None], None, np.zeros((1, 2)), np.zeros((1, 2)), [0])
    with pytest.raises(ValueError):
        adapt.walk_distances_runs(np.zeros((2, 2)), [0, 2], np.eye(2)[None], None, np.zeros((1, 2)), np.zeros((1, 2)), [1])
    with pytest.raises(ValueError):
        adapt.check_settings("nope", 3, None, None)
    with pytest.raises(ValueError):
        adapt.check_settings("move-distance", 3, 4, None)
    assert adapt.check_settings("move-distance", 3, None, None) == (3, adapt.MAX_NSTEPS)


# ---- the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f,c,want", [
    (20, 0, 0, 20),           # nobody counted: unchanged
    (20, 4, 10, 22),          # 2f < c: longer by a tenth
    (5, 0, 10, 6),            # ... by at least one
    (995, 0, 10, 1000),       # ... never above max
    (1000, 0, 10, 1000),
    (20, 8, 10, 18),          # 4f >= 3c: shorter by a tenth
    (20, 15, 20, 18),         # (4f == 3c counts as far enough)
    (4, 10, 10, 3),           # ... by at least one
    (3, 10, 10, 3),           # ... never below min
    (20, 5, 10, 20),          # in between: unchanged
    (20, 7, 10, 20),
])
def test_rule_steps_and_clamps(n, f, c, want):
    assert adapt.next_nsteps(n, f, c, 3, 1000) == want
    got = adapt.next_nsteps(np.array([n, n]), np.array([f, f]), np.array([c, c]), 3, 1000)
    assert list(got) == [want, want]


def test_far_fraction_is_nan_without_counted_walkers():
    ff = adapt.far_fraction([1, 0], [4, 0])
    assert ff[0] == 0.25 and np.isnan(ff[1])


# ---- the drivers ------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall
    assert a.logz == b.logz and a.logzerr == b.logzerr and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)
    assert np.array_equal(a.logl_birth, b.logl_birth)


KW = dict(nlive=120, kbatch=10, nsteps=3, dlogz=0.1, max_calls=400_000)


@pytest.mark.parametrize("clustering", [False, True])
def test_pinned_adaptive_run_is_the_plain_run(clustering):
    plain = run_nested_slice(prior, loglike, 2, seed=4, clustering=clustering, **KW)
    got = run_nested_slice(prior, loglike, 2, seed=4, clustering=clustering, adaptive_nsteps="move-distance",
                           min_nsteps=3, max_nsteps=3, **KW)
    _same(got, plain)
    assert plain.nsteps_trace is None and plain.far_fraction is None
    assert got.nsteps_trace.shape == (got.niter // KW["kbatch"],) and np.all(got.nsteps_trace == 3)
    assert got.far_fraction.shape == got.nsteps_trace.shape
    assert np.all((got.far_fraction >= 0) & (got.far_fraction <= 1))


def walk(cube, theta, logl, lstar, chol, wrapped, nsteps, max_rounds, seed):
    """A deterministic constrained move (tests/test_nested_ensemble_host.py's) whose reach grows with nsteps."""
    rng = np.random.default_rng(seed)
    c = cube.copy()
    used = 0
    for _ in range(nsteps):
        prop = np.clip(c + (rng.standard_normal(c.shape) @ chol.T) * 0.5, 0.0, np.nextafter(1.0, 0.0))
        ok = loglike(prior(prop)) > lstar
        used += len(c) + int(np.sum(~ok))
        c[ok] = prop[ok]
    th = prior(c)
    return c, th, loglike(th), used


class _WalkerRuns:
    """walker_runs taking an int or a per-group step count, as GpuRVModel.slice_walk_runs does."""

    def __init__(self):
        self.steps = []

    def __call__(self, cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
        R = len(run_start) - 1
        steps = np.broadcast_to(np.asarray(nsteps), (R,))
        self.steps.append(nsteps)
        cube, theta, logl = cube.copy(), theta.copy(), logl.copy()
        ncalls = np.zeros(R, dtype=np.int64)
        for r in range(R):
            rows = slice(run_start[r], run_start[r + 1])
            cube[rows], theta[rows], logl[rows], ncalls[r] = walk(cube[rows], theta[rows], logl[rows], lstar[r], chol[r],
                                                                  wrapped, int(steps[r]), max_rounds, seeds[r])
        return cube, theta, logl, ncalls


def test_pinned_walker_paths_are_the_plain_runs():
    for kw in (dict(walker=walk), dict(walker_runs=_WalkerRuns())):
        plain = run_nested_slice(prior, loglike, 3, seed=8, **kw, **KW)
        got = run_nested_slice(prior, loglike, 3, seed=8, adaptive_nsteps="move-distance", max_nsteps=3, **kw, **KW)
        _same(got, plain)


@pytest.mark.parametrize("clustering", [False, True])
def test_adaptive_ensemble_is_the_standalone_runs(clustering):
    seeds = (21, 22, 23, 24)
    kw = dict(KW, nsteps=1, dlogz=0.3)
    wr = _WalkerRuns()
    got = run_nested_ensemble(prior, loglike, 3, seeds, walker_runs=wr, clustering=clustering,
                              adaptive_nsteps="move-distance", **kw)
    for s, g in zip(seeds, got):
        one = run_nested_slice(prior, loglike, 3, seed=s, walker_runs=_WalkerRuns(), clustering=clustering,
                               adaptive_nsteps="move-distance", **kw)
        _same(g, one)
        assert np.array_equal(g.nsteps_trace, one.nsteps_trace)
        assert np.array_equal(g.far_fraction, one.far_fraction, equal_nan=True)
    # the runs' step counts part ways, and the walk calls then get them per group
    assert any(not np.isscalar(s) and not isinstance(s, int) for s in wr.steps)
    assert max(int(g.nsteps_trace.max()) for g in got) > 1


def test_walker_path_equals_walker_runs_path():
    kw = dict(KW, nsteps=2)
    a = run_nested_slice(prior, loglike, 3, seed=9, walker=walk, adaptive_nsteps="move-distance", **kw)
    b = run_nested_slice(prior, loglike, 3, seed=9, walker_runs=_WalkerRuns(), adaptive_nsteps="move-distance", **kw)
    _same(a, b)
    assert np.array_equal(a.nsteps_trace, b.nsteps_trace)


def test_correlated_gaussian_lengthens_the_walk():
    ndim = 10
    rng = np.random.default_rng(5)
    A = rng.standard_normal((ndim, ndim))
    cov = A @ A.T + 0.05 * np.eye(ndim)
    cov = cov / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))      # correlations up to ~0.99, unit variances
    icov = np.linalg.inv(cov)
    _, logdet = np.linalg.slogdet(cov)
    lnz = ndim * LNZ_1D                                            # (the log-L is normalised to (2 pi)^(ndim / 2))

    def ll(x):
        return -0.5 * np.einsum("ni,ij,nj->n", x, icov, x) - 0.5 * logdet

    res = run_nested_slice(prior, ll, ndim, nlive=200, kbatch=20, nsteps=1, dlogz=0.1, seed=2,
                           adaptive_nsteps="move-distance", max_nsteps=60)
    assert res.nsteps_trace[0] == 1 and res.nsteps_trace.max() > 1
    assert abs(res.logz - lnz) < 3 * res.logzerr, (res.logz, lnz, res.logzerr)


@pytest.mark.parametrize("ndim,nlive", [(1, 100), (2, 500)])
def test_gaussian_known_answers_with_adaptation(ndim, nlive):
    res = run_nested_slice(prior, loglike, ndim, nlive=nlive, dlogz=0.05, seed=1, adaptive_nsteps="move-distance")
    want = ndim * LNZ_1D                                             # -2.0768 in 1-D, -4.1536 in 2-D
    assert abs(res.logz - want) < 4 * res.logzerr + 0.05
    assert res.nsteps_trace.min() >= 3 * ndim


def test_resident_live_sets_refuse_adaptation():
    with pytest.raises(ValueError, match="adaptive_nsteps"):
        run_nested_slice(None, None, 2, live=object(), adaptive_nsteps="move-distance")
    with pytest.raises(ValueError, match="adaptive_nsteps"):
        run_nested_ensemble(None, None, 2, [1], live=object(), adaptive_nsteps="move-distance")
