"""CPU: PolyChord's stepping-out slice proposal (evidence_amd/stepout.py) as the host walk of run_nested_slice
runs it — the basis, the bracket's expansion against hand-built slices, uniformity without a constraint, the reference's
Gaussian known answers — PolyChord's precision_criterion stop rule, and the settings mapping polychord_kwargs."""
import numpy as np
import pytest
from scipy import stats

from evidence_amd import stepout
from evidence_amd.nested import polychord_kwargs, run_nested_slice

LNZ_1D = float(np.log(np.sqrt(2 * np.pi) / 20.0))       # -2.0768 (tests/test_polychord.py of the reference)


def test_basis_is_orthonormal_and_its_vectors_cycle_with_the_move():
    rng = np.random.default_rng(1)
    q = stepout.gram_schmidt(rng.standard_normal((50, 7, 7)))
    eye = np.einsum("kij,klj->kil", q, q)
    assert np.abs(eye - np.eye(7)).max() < 1e-12
    # the walk draws a fresh basis at every m mod D == 0 and moves along its vectors in turn: with a flat log-L, a unit factor
    # and a bracket wider than the cube (both ends on the walls at once, the first shrink point accepted), move m's
    # displacement is a multiple of q_{m mod D}
    D = 3
    seen = []

    def evaluate(c):
        seen.append(c.copy())
        return c, np.zeros(len(c))
    wu = np.full((1, D), 0.5)
    stepout.walk(wu, wu.copy(), np.zeros(1), -np.inf, np.eye(D), None, 2 * D, 100, 10.0, np.random.default_rng(4), evaluate)
    assert len(seen) == 2 * D
    r = np.random.default_rng(4)                 # replay: the basis at m = 0 and m = D, then v and one shrink uniform a move
    pos = np.full(D, 0.5)
    for m in range(2 * D):
        if m % D == 0:
            qb = stepout.gram_schmidt(r.standard_normal((1, D, D)))[0]
        r.random(1)
        r.random(1)
        step = seen[m][0] - pos
        assert abs(abs(step @ qb[m % D]) - np.linalg.norm(step)) < 1e-12
        pos = seen[m][0]


def _slice_1d(lo_in, hi_in, calls):
    def evaluate(c):
        calls.append(c[:, 0].copy())
        x = c[:, 0]
        return c, np.where((x > lo_in) & (x < hi_in), 0.0, -1.0)
    return evaluate


def test_stepping_out_expands_by_whole_widths_and_walls_cost_no_call():
    # 1-D slice (0.2, 0.8) in the unit cube, walker at 0.5, width 0.1: the right end steps out by whole widths until one is
    # outside the slice, then the left end does; every evaluated end is a call
    g = np.random.default_rng(7)                             # the walk's draws: the 1 x 1 basis normal, then v
    sign = np.sign(g.standard_normal((1, 1, 1))[0, 0, 0])
    v = g.random(1)[0]
    lo0, hi0 = -0.1 * v, -0.1 * v + 0.1
    calls = []
    wu = np.array([[0.5]])
    stepout.walk(wu, wu.copy(), np.zeros(1), -0.5, np.eye(1), None, 1, 1000, 0.1, np.random.default_rng(7),
                 _slice_1d(0.2, 0.8, calls))
    x = np.concatenate(calls)
    inside = lambda t: (0.5 + sign * t > 0.2) & (0.5 + sign * t < 0.8)
    right = hi0 + 0.1 * np.arange(20)
    left = lo0 - 0.1 * np.arange(20)
    nr = int(np.argmax(~inside(right))) + 1                  # the ends inside, and the first one outside
    nl = int(np.argmax(~inside(left))) + 1
    assert np.allclose(x[:nr], 0.5 + sign * right[:nr], rtol=0, atol=1e-12)        # (the walk adds w end by end)
    assert np.allclose(x[nr:nr + nl], 0.5 + sign * left[:nl], rtol=0, atol=1e-12)
    assert nr + nl == 8                                      # 0.3 to either side of 0.5: three widths inside, one out, each
    assert 0.2 < wu[0, 0] < 0.8                              # the shrink ends inside the slice
    # a slice wider than the cube: the ends step out to the walls and stop there; the end ON a wall is out, without a call
    calls = []
    wu = np.array([[0.5]])
    n = stepout.walk(wu, wu.copy(), np.zeros(1), -0.5, np.eye(1), None, 1, 1000, 0.1, np.random.default_rng(7),
                     _slice_1d(-1.0, 2.0, calls))
    ends = np.concatenate(calls)[:-1]                        # (the last call: the accepted shrink point)
    assert n == len(calls) and np.all((ends > 0.0) & (ends < 1.0))
    assert n == 5 + 5 + 1                                    # 0.5 to a wall: five ends inside each way, the sixth clamped
    assert 0.0 <= wu[0, 0] < 1.0


def test_wrapped_coordinates_set_no_limit():
    # 1 wall coordinate (direction 0 along it) and 1 wrapped one: the wall chord is unbounded, and the bracket steps out past
    # the half turn the chord walk would stop at
    u = np.array([[0.5, 0.5]])
    d = np.array([[0.0, 1.0]])
    cmin, cmax = stepout.wall_chord(u, d, np.array([False, True]))
    assert cmin[0] == -np.inf and cmax[0] == np.inf
    cmin, cmax = stepout.wall_chord(u, np.array([[0.5, 1.0]]), np.array([False, True]))
    assert (cmin[0], cmax[0]) == (-1.0, 1.0)


@pytest.mark.parametrize("ndim", [2, 3])
def test_unconstrained_walk_is_uniform_in_the_cube(ndim):
    rng = np.random.default_rng(11)
    k = 4000
    wrapped = np.zeros(ndim, dtype=bool)
    wrapped[-1] = True
    wu = np.full((k, ndim), 0.31)
    chol = np.linalg.cholesky(np.diag(np.linspace(0.05, 0.2, ndim) ** 2))
    n = stepout.walk(wu, wu.copy(), np.zeros(k), -np.inf, chol, wrapped, 6 * ndim, 1000, 1.0, rng,
                     lambda c: (c, np.zeros(len(c))))
    assert n > 6 * ndim * k
    for j in range(ndim):
        assert stats.kstest(wu[:, j], "uniform").pvalue > 1e-3, j


@pytest.mark.parametrize("ndim,nlive", [(1, 200), (2, 400)])
def test_gaussian_known_answers(ndim, nlive):
    prior = lambda cube: -10.0 + 20.0 * cube
    loglike = lambda x: -0.5 * np.sum(x * x, axis=1)
    res = run_nested_slice(prior, loglike, ndim, nlive=nlive, dlogz=0.05, seed=5, proposal="stepout", nsteps=5 * ndim)
    want = ndim * LNZ_1D                                     # -2.0768, -4.1536
    assert abs(res.logz - want) < 0.5
    assert abs(res.logz - want) < 4 * res.logzerr + 0.1, (res.logz, want, res.logzerr)


def _ratio(res, kbatch, nlive):
    """Z_live / (Z_dead + Z_live) at the end of a run, from its result arrays."""
    ndead = res.niter
    logz_final = res.logz
    lz_dead = np.logaddexp.reduce(res.logwt[:ndead]) + logz_final
    logx = -np.sum(np.tile(1.0 / (nlive - np.arange(kbatch)), ndead // kbatch))
    ll = np.sort(res.logl[ndead:])
    lz_live = logx + ll[-1] + np.log(np.mean(np.exp(ll - ll[-1])))
    return np.exp(lz_live - np.logaddexp(lz_dead, lz_live))


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_precision_criterion_stops_where_the_definition_says(proposal):
    prior = lambda cube: -10.0 + 20.0 * cube
    loglike = lambda x: -0.5 * np.sum(x * x, axis=1)
    kw = dict(nlive=100, kbatch=10, seed=3, proposal=proposal, nsteps=6)
    res = run_nested_slice(prior, loglike, 2, precision_criterion=0.01, **kw)
    assert _ratio(res, 10, 100) < 0.01
    before = run_nested_slice(prior, loglike, 2, precision_criterion=0.01, max_iter=res.niter - 10, **kw)
    assert before.niter == res.niter - 10 and _ratio(before, 10, 100) >= 0.01
    assert np.array_equal(before.logl[:before.niter], res.logl[:before.niter])      # the same run, stopped earlier


def test_polychord_kwargs_map_the_settings():
    kw = polychord_kwargs(3)
    assert kw == {"nlive": 75, "nsteps": 15, "clustering": True, "precision_criterion": 0.001, "proposal": "stepout"}
    kw = polychord_kwargs(2, {"nlive": 60, "num_repeats": 4, "do_clustering": False, "precision_criterion": 0.01,
                              "feedback": 0, "write_resume": True})
    assert kw == {"nlive": 60, "nsteps": 4, "clustering": False, "precision_criterion": 0.01, "proposal": "stepout"}
    with pytest.raises(ValueError):
        polychord_kwargs(2, {"boost_posterior": 5.0})
    with pytest.raises(TypeError):
        polychord_kwargs(2, {"nlive": 60.0})
    prior = lambda cube: -10.0 + 20.0 * cube
    loglike = lambda x: -0.5 * np.sum(x * x, axis=1)
    res = run_nested_slice(prior, loglike, 1, seed=2, **dict(polychord_kwargs(1, {"nlive": 100}), clustering=False))
    assert abs(res.logz - LNZ_1D) < 0.5


def test_chord_spelled_out_is_the_default_bit_for_bit():
    prior = lambda cube: -10.0 + 20.0 * cube
    loglike = lambda x: -0.5 * np.sum(x * x, axis=1)
    a = run_nested_slice(prior, loglike, 2, nlive=100, seed=9, dlogz=0.5)
    b = run_nested_slice(prior, loglike, 2, nlive=100, seed=9, dlogz=0.5, proposal="chord", step_width=1.0)
    assert a.logz == b.logz and a.ncall == b.ncall and np.array_equal(a.samples, b.samples)
    with pytest.raises(ValueError):
        run_nested_slice(prior, loglike, 2, nlive=100, proposal="slice")
    with pytest.raises(ValueError):
        run_nested_slice(prior, loglike, 2, nlive=100, proposal="stepout", step_width=0.0)
