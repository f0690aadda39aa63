"""CPU: the MLFriends clustering of the survivors (evidence_amd/clustering.py) and nested sampling that whitens
each mode's walk with that mode's own covariance (run_nested_slice / run_nested_ensemble(clustering=True)): known partitions,
canonical labels, batched = per run, a bimodal known answer, bit identity with clustering off where one cluster is found,
and an ensemble that is its standalone runs."""
import numpy as np
import pytest

from evidence_amd import run_nested_ensemble
from evidence_amd.clustering import cluster_runs, keep_words
from evidence_amd.nested import run_nested_slice


def _blobs(rng, centres, n, sigma, ndim):
    return np.concatenate([np.clip(rng.normal(c, sigma, (n, ndim)), 0.0, np.nextafter(1.0, 0.0)) for c in centres])


def _one(u, scale=None, wrapped=None, nboot=30, seed=7):
    scale = np.ones(u.shape[1]) if scale is None else scale
    labels, ncl, r2 = cluster_runs(u, [0, len(u)], scale[None, :], wrapped, nboot, [seed])
    return labels, int(ncl[0]), float(r2[0])


@pytest.mark.parametrize("nboot", [0, 1, 30, 32])
def test_three_separated_blobs_are_three_clusters(nboot):
    rng = np.random.default_rng(1)
    u = _blobs(rng, [0.2, 0.5, 0.8], 80, 0.02, 3)
    perm = rng.permutation(len(u))
    labels, ncl, r2 = _one(u[perm], nboot=nboot)
    assert ncl == 3 and r2 > 0
    truth = (np.arange(len(u)) // 80)[perm]
    for c in range(3):                                   # every cluster is exactly one blob
        assert len(set(truth[labels == c])) == 1
    # canonical labels: row 0 in cluster 0, clusters numbered in the order of their smallest row
    firsts = [np.flatnonzero(labels == c)[0] for c in range(3)]
    assert labels[0] == 0 and firsts == sorted(firsts)


def test_a_blob_across_the_wrap_is_one_cluster_only_when_wrapped():
    rng = np.random.default_rng(2)
    u = rng.normal(0.0, 0.02, (150, 2)) + np.array([0.0, 0.5])
    u[:, 0] %= 1.0                                       # half of the blob near 0, half near 1
    assert _one(u, wrapped=[True, False])[1] == 1
    assert _one(u, wrapped=None)[1] == 2
    assert _one(u, wrapped=[False, False])[1] == 2


def test_uniform_rows_are_one_cluster():
    rng = np.random.default_rng(3)
    for ndim, n in ((1, 100), (3, 300), (7, 400)):
        assert _one(rng.random((n, ndim)))[1] == 1


def test_small_runs_and_the_radius_rules():
    rng = np.random.default_rng(4)
    u = rng.random((3, 2))
    labels, ncl, r2 = cluster_runs(u, [0, 0, 1, 3], np.ones((3, 2)), None, 30, [1, 2, 3])
    assert list(ncl) == [0, 1, 1] and r2[0] == 0.0 and r2[1] == 0.0
    assert list(labels) == [0, 0, 0]
    # two rows: every bootstrap keeps both or neither or splits them; a split's radius is their distance, and with no split
    # the nearest-neighbour fallback gives the same distance: one cluster
    d2 = float(np.sum((u[1] - u[2]) ** 2))
    assert r2[2] == d2
    # without bootstraps: the largest nearest-neighbour distance
    labels, ncl, r2 = cluster_runs(np.array([[0.1], [0.2], [0.9]]), [0, 3], [[1.0]], None, 0, [0])
    assert r2[0] == (0.9 - 0.2) ** 2 and ncl[0] == 1


def test_keep_bits_are_the_uniform01_words():
    """Bit 63 - b of the splitmix64 word: the draw uniform01(seed, i) < 2^-1 decides bit 63, i.e. bootstrap 0."""
    z = keep_words(12345, 1000)
    u01 = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert np.array_equal(u01 >= 0.5, ((z >> np.uint64(63)) & np.uint64(1)).astype(bool))


def test_batched_call_is_the_runs_one_by_one_and_deterministic():
    rng = np.random.default_rng(5)
    runs = [_blobs(rng, [0.3, 0.7], 60, 0.03, 4), rng.random((0, 4)), rng.random((1, 4)), rng.random((2, 4)),
            rng.random((200, 4)), _blobs(rng, [0.2, 0.5, 0.8], 40, 0.01, 4)]
    cube = np.concatenate(runs)
    run_start = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    scale = rng.uniform(0.5, 3.0, (len(runs), 4))
    seeds = [11, 2 ** 64 - 1, 0, 5, 9, 2 ** 63]
    wrapped = [False, True, False, False]
    got = cluster_runs(cube, run_start, scale, wrapped, 30, seeds)
    again = cluster_runs(cube, run_start, scale, wrapped, 30, seeds)
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
    for r in range(len(runs)):
        lab, ncl, r2 = cluster_runs(runs[r], [0, len(runs[r])], scale[r:r + 1], wrapped, 30, [seeds[r]])
        assert np.array_equal(got[0][run_start[r]:run_start[r + 1]], lab)
        assert got[1][r] == ncl[0] and got[2][r].tobytes() == r2[0].tobytes()
    assert list(got[1][:4]) == [2, 0, 1, 1] and got[1][5] == 3


def test_argument_errors():
    u = np.random.default_rng(6).random((10, 2))
    with pytest.raises(ValueError):
        cluster_runs(u, [0, 10], np.ones((1, 2)), None, 33, [0])
    with pytest.raises(ValueError):
        cluster_runs(u, [0, 6, 4, 10], np.ones((3, 2)), None, 30, [0, 1, 2])
    with pytest.raises(ValueError):
        cluster_runs(u, [1, 10], np.ones((1, 2)), None, 30, [0])
    with pytest.raises(ValueError):
        cluster_runs(u, [0, 10], np.array([[1.0, 0.0]]), None, 30, [0])
    with pytest.raises(ValueError):
        cluster_runs(u, [0, 10], np.array([[1.0, np.inf]]), None, 30, [0])


# ---- nested sampling with clustering -------------------------------------------------------------------------------------
SIG = 0.02
C1, C2 = np.full(3, 0.3), np.full(3, 0.7)
_CORR = np.array([[1.0, 0.9, 0.9], [0.9, 1.0, 0.9], [0.9, 0.9, 1.0]])
_FLIP = np.diag([1.0, -1.0, 1.0])
COV1, COV2 = SIG ** 2 * _CORR, SIG ** 2 * _FLIP @ _CORR @ _FLIP          # correlations +0.9, and +-0.9


def _gauss_logpdf(x, c, cov):
    d = x - c
    sol = np.linalg.solve(cov, d.T).T
    return -0.5 * np.sum(d * sol, axis=1) - 0.5 * np.log(np.linalg.det(2 * np.pi * cov))


def mixture_loglike(x):
    return np.logaddexp(_gauss_logpdf(x, C1, COV1), _gauss_logpdf(x, C2, COV2)) + np.log(0.5)


def identity_prior(cube):
    return np.array(cube, dtype=np.float64)


def test_bimodal_mixture_known_answer_with_clustering():
    """Two narrow, differently correlated Gaussians of equal weight in the unit cube: Z = 1.  Both modes keep their
    share of the posterior, and the last iterations see them as separate clusters."""
    r = run_nested_slice(identity_prior, mixture_loglike, 3, nlive=300, seed=3, clustering=True)
    assert abs(r.logz) < 4 * r.logzerr + 0.1, (r.logz, r.logzerr)
    w = np.exp(r.logwt)
    near1 = np.linalg.norm(r.samples - C1, axis=1) < np.linalg.norm(r.samples - C2, axis=1)
    assert 0.35 <= np.sum(w[near1]) <= 0.65 and 0.35 <= np.sum(w[~near1]) <= 0.65
    assert r.nclusters is not None and len(r.nclusters) > 0 and r.nclusters[-1] >= 2


def gauss_prior(cube):
    return -10.0 + 20.0 * cube


def gauss_loglike(x):
    return -0.5 * np.sum(x * x, axis=1)


def _walk(cube, theta, logl, lstar, chol, wrapped, nsteps, max_rounds, seed, prior=gauss_prior, loglike=gauss_loglike):
    """A crude but deterministic constrained move whose call count depends on the seed (rejections cost extra)."""
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
    """A numpy stand-in for GpuRVModel.slice_walk_runs: _walk group by group; records the group count of every call."""

    def __init__(self, prior, loglike):
        self.prior, self.loglike, self.groups = prior, loglike, []

    def __call__(self, cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
        R = len(run_start) - 1
        assert len(lstar) == R and chol.shape[0] == R and len(seeds) == R and run_start[-1] == len(cube)
        self.groups.append(R)
        cube, theta, logl = cube.copy(), theta.copy(), logl.copy()
        ncalls = np.zeros(R, dtype=np.int64)
        for r in range(R):
            rows = slice(run_start[r], run_start[r + 1])
            cube[rows], theta[rows], logl[rows], ncalls[r] = _walk(cube[rows], theta[rows], logl[rows], lstar[r], chol[r],
                                                                   wrapped, nsteps, max_rounds, seeds[r], self.prior, self.loglike)
        return cube, theta, logl, ncalls


def _same(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall
    assert a.logz == b.logz and a.logzerr == b.logzerr and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)


def test_one_cluster_every_iteration_is_the_unclustered_run():
    kw = dict(nlive=160, kbatch=20, nsteps=4, dlogz=0.1, max_calls=500_000)
    # the host walk
    off = run_nested_slice(gauss_prior, gauss_loglike, 3, seed=4, **kw)
    on = run_nested_slice(gauss_prior, gauss_loglike, 3, seed=4, clustering=True, **kw)
    _same(on, off)
    assert off.nclusters is None and len(on.nclusters) > 0
    assert np.all(on.nclusters == 1)
    # walker_runs with the walkers grouped by cluster against the one-factor walker
    single = lambda *a: _walk(*a)                                        # noqa: E731
    off = run_nested_slice(gauss_prior, gauss_loglike, 3, seed=5, walker=single, **kw)
    wr = _WalkerRuns(gauss_prior, gauss_loglike)
    on = run_nested_slice(gauss_prior, gauss_loglike, 3, seed=5, clustering=True, walker_runs=wr, **kw)
    _same(on, off)
    assert np.all(on.nclusters == 1) and set(wr.groups) == {1}


def _mix_prior(cube):
    return identity_prior(cube)


def test_clustered_ensemble_is_its_standalone_clustered_runs():
    kw = dict(nlive=150, kbatch=30, nsteps=3, dlogz=0.5, max_calls=300_000)
    seeds = [3, 8, 21]
    wr = _WalkerRuns(_mix_prior, mixture_loglike)
    ens = run_nested_ensemble(_mix_prior, mixture_loglike, 3, seeds, walker_runs=wr, clustering=True, **kw)
    assert max(wr.groups) > len(seeds)                                    # some call had more walk groups than runs
    for s, got in zip(seeds, ens):
        one = run_nested_slice(_mix_prior, mixture_loglike, 3, seed=s, clustering=True,
                               walker_runs=_WalkerRuns(_mix_prior, mixture_loglike), **kw)
        _same(got, one)
        assert np.array_equal(got.nclusters, one.nclusters)
    assert max(int(np.max(r.nclusters)) for r in ens) >= 2


def test_clustering_argument_errors():
    with pytest.raises(ValueError, match="walker_runs"):
        run_nested_slice(gauss_prior, gauss_loglike, 2, nlive=50, clustering=True, walker=lambda *a: _walk(*a))
    with pytest.raises(ValueError, match="live"):
        run_nested_slice(None, None, 2, nlive=50, clustering=True, live=object())
    with pytest.raises(ValueError):
        run_nested_slice(gauss_prior, gauss_loglike, 2, nlive=50, clustering=True, nboot=33)
