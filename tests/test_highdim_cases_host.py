"""CPU: the references of the high-dimensional walk and live-set tests (tests/highdim_cases.py) meet, alone, every condition
test_gpu_walk_highdim.py and test_gpu_live_highdim.py rely on — the float64 replay of every walk case stays within
walk_replay.SPREAD of the longdouble replay with the fragile share under the cap and TOL_U * scale under the ceiling
(test_walk_replay_host.py's test, at 48 .. 129 parameters); the float64 numpy factor stays within a few 1e-16 of the longdouble
factor, which is what the device's bound is 64 times of; the sort model's live set has log-L of both signs and exact ties; and
the walk kernel's LDS pointer chain ends inside walk_lds_bytes at every slot count walk_args can choose at 48, 49, 64 and 129
parameters.  The figures are printed (pytest -s) and kept in profiles/highdim_replay.txt."""
import numpy as np
import pytest

import highdim_cases as hc
import walk_replay as wr
from evidence_amd.nested import _whitening
from test_walk_replay_host import start


def _print(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _check(name, proposal, states, ncalls, ev, wrapped, capsys, **walk):
    fig = wr.check_prefixes(states, ncalls, ev, tol_u=wr.TOL_U, wrapped=wrapped, proposal=proposal, **walk)
    _print(capsys, f"host replay {name:22s} {proposal:8s} pairs {fig.pairs:6d} fragile {fig.fragile:3d} loose {fig.loose:3d} exact moves "
                   f"{fig.exact_moves:3d} spread/scale {fig.spread:.2e} worst {fig.worst_abs:.2e} max scale {fig.max_scale:8.1f} "
                   f"TOL_U*scale {wr.TOL_U * fig.max_scale:.1e}")
    assert fig.spread <= wr.SPREAD and fig.worst <= fig.spread
    assert fig.fragile + fig.loose <= wr.FRAGILE_CAP * fig.pairs
    assert wr.TOL_U * fig.max_scale <= wr.TOL_CEILING
    if proposal == "chord":
        assert fig.max_scale == 1.0
    return fig


@pytest.mark.parametrize("name", [c.name for c in hc.WALK_CASES])
def test_float64_and_longdouble_replays_agree_at_high_dimension(name, capsys):
    c = hc.WALK_CASE[name]
    ev, wrapped = hc.gaussian_evaluator(c.ndim), hc.wrapped(c.ndim)
    cube, theta, logl, lstar, chol = start(ev, c.ndim, c.k, c.seed, 0.5)
    assert len(cube) == c.k // 2
    walk = dict(seed=7, wid=np.arange(len(cube)), lstar=lstar, chol=chol, max_rounds=200, step_width=1.0)
    states, ncalls, _ = wr.walk(cube, theta, logl, c.nsteps, proposal=c.proposal, wrapped=wrapped, evaluate=ev, **walk)
    fig = _check(name, c.proposal, states, ncalls, ev, wrapped, capsys, **walk)
    assert fig.pairs == c.nsteps * len(cube)
    # the walkers move: a case in which nothing was accepted would compare nothing
    assert np.mean(np.any(states[-1][0] != cube, axis=1)) > 0.9


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_run_mode_replays_agree_at_64_parameters(proposal, capsys):
    c = hc.RUN_MODE
    ev, wrapped = hc.gaussian_evaluator(c.ndim), hc.wrapped(c.ndim)
    cube, theta, logl, lstar, chol = start(ev, c.ndim, c.k, c.seed, 0.5)
    sizes, steps = np.array(c.sizes), np.array(c.steps)
    assert len(cube) == sizes.sum()
    groups = np.repeat(np.arange(4), sizes)
    lst, chols, seeds = hc.run_mode_arguments(lstar, chol)
    kw = dict(seed=seeds[groups], lstar=lst[groups], wid=np.concatenate([np.arange(n) for n in sizes]), chol=chols[groups],
              max_rounds=200, step_width=0.8)
    states, calls = [(cube, theta, logl)], [np.zeros(4, dtype=np.int64)]
    for n in range(1, steps.max() + 1):
        on = steps[groups] >= n
        r = wr.replay_move(*[a[on] for a in states[-1]], n - 1, proposal=proposal, wrapped=wrapped, evaluate=ev, dtype=np.float64,
                           **{key: (v[on] if np.ndim(v) else v) for key, v in kw.items()})
        u, t, l = (a.copy() for a in states[-1])
        u[on], t[on], l[on] = r.u, r.theta, r.logl
        states.append((u, t, l))
        calls.append(calls[-1] + np.bincount(groups[on], weights=r.calls, minlength=4).astype(np.int64))
    fig = _check("D64 run mode", proposal, states, calls, ev, wrapped, capsys, groups=groups, steps=steps, **kw)
    assert fig.pairs == int(np.sum(sizes * steps))


@pytest.mark.parametrize("ndim, proposal", [(49, "chord"), (49, "stepout"), (129, "chord")])
def test_resident_step_replays_agree(ndim, proposal, capsys):
    c = hc.LIVE_STEP
    ev, wrapped = hc.gaussian_evaluator(ndim), hc.wrapped(ndim)
    cube, order, lstar, rows = hc.live_step_case(ndim, lambda u: ev(u)[1])
    theta, logl = ev(cube)
    chol = _whitening(cube[order[c.kdead:]])
    walk = dict(seed=c.seed, wid=np.arange(c.kdead) + c.base, lstar=lstar, chol=chol, max_rounds=200, step_width=1.0)
    states, ncalls, _ = wr.walk(cube[rows], theta[rows], logl[rows], c.nsteps, proposal=proposal, wrapped=wrapped, evaluate=ev, **walk)
    fig = _check(f"D{ndim} live step", proposal, states, ncalls, ev, wrapped, capsys, **walk)
    assert fig.pairs == c.nsteps * c.kdead


@pytest.mark.parametrize("ndim, nsurv", hc.FACTOR_CASES)
def test_float64_factor_against_the_longdouble_factor(ndim, nsurv, capsys):
    """The distance the device's bound is FACTOR_MARGIN times of, per case; with it the bound stays the derived one (under the
    floor of 1e-12), and the factor is well conditioned: its smallest diagonal is a tenth of a uniform coordinate's spread."""
    ev = hc.gaussian_evaluator(ndim)
    cube = hc.live_cube(ndim, nsurv)
    _, rows = hc.survivors_of(cube, ev(cube)[1])
    assert rows.shape == (nsurv, ndim)
    bound, host, ref = hc.factor_bound(rows)
    diag = float(np.diag(ref).min())
    _print(capsys, f"host factor D {ndim:3d} n {nsurv:4d}: float64 - longdouble {host:.2e} of max|L|, device bound {bound:.2e}, "
                   f"max|L| {float(np.abs(ref).max()):.3f}, smallest diagonal {diag:.3f}")
    assert 0 < host and hc.FACTOR_MARGIN * host <= hc.FACTOR_FLOOR and bound == hc.FACTOR_MARGIN * host
    assert diag > 0.03 and np.all(np.triu(ref, 1) == 0)
    # the reference is the factor of its own covariance: L L^T against the float64 covariance, to float64's rounding
    d = rows - rows.mean(axis=0)
    cov = d.T @ d / (nsurv - 1) + 1e-14 * np.eye(ndim)
    assert np.abs((ref @ ref.T).astype(np.float64) - cov).max() <= 1e-13 * np.abs(cov).max()


def test_factor_reference_is_the_textbook_factor_at_7_parameters():
    rows = np.random.default_rng(5).random((40, 7))
    d = rows - rows.mean(axis=0)
    assert np.allclose(hc.factor_reference(rows).astype(np.float64), np.linalg.cholesky(d.T @ d / 39 + 1e-14 * np.eye(7)), rtol=1e-13, atol=1e-15)


def test_the_sort_models_live_set_has_both_signs_and_exact_ties():
    ev = hc.gaussian_evaluator(hc.SORT_NDIM, hc.SORT_SVRAD)
    cube = hc.sort_cube(400, 40, 31)
    logl = ev(cube)[1]
    assert (logl > 0).sum() > 40 and (logl < 0).sum() > 40
    assert len(np.unique(logl)) <= 360 and np.array_equal(logl[360:], ev(cube[360:])[1])
    order = np.argsort(logl, kind="stable")
    tied = np.flatnonzero(np.diff(logl[order]) == 0)
    assert tied.size >= 40 and np.all(order[tied] < order[tied + 1])           # ties by row: what the device has to reproduce


@pytest.mark.parametrize("stepout", [False, True])
def test_the_walk_kernels_pointer_chain_ends_inside_its_lds(stepout, capsys):
    """At every slot count walk_args can end on (1 .. what it shrinks 32 to) for 48, 49, 64 and 129 parameters: the last byte the
    kernel's pointers reach lies within walk_lds_bytes, the walk's 3 PB D doubles fit the tile's window, PB D <= 1024 and the
    whole is within the 64 KiB a launch may ask for.  (A layout fault is found by this arithmetic, not by a launch.)"""
    for ndim in (48, 49, 64, 129):
        if stepout and ndim > 64:
            continue
        top = hc.walk_slots(ndim, stepout)
        assert top >= 1
        for pb in range(1, top + 1):
            size, end, need, window = hc.walk_lds(pb, ndim, stepout)
            assert end <= size <= 64 * 1024 and need <= window and pb * ndim <= 1024, (ndim, pb)
        size, end, need, window = hc.walk_lds(top, ndim, stepout)
        _print(capsys, f"walk LDS D {ndim:3d} {'stepout' if stepout else 'chord':8s} slots (asked 32) {top:2d}: walk_lds_bytes {size:6d}, chain ends at "
                       f"{end:6d}, window {window:5d} doubles for 3 PB D = {need:5d}, factor {'in LDS' if ndim <= hc.K_WALK_CHOL_LDS else 'global'}")
    # what bounds the slots is the LDS (a slot of this model takes 8 D doubles and more, so 60 KiB end before PB D = 1024 does);
    # the factor staged at 48 costs 18 KiB: fewer slots than at 49
    assert hc.walk_slots(48, stepout) < hc.walk_slots(49, stepout) and hc.walk_lds(hc.walk_slots(49, stepout) + 1, 49, stepout)[0] > 60 * 1024


def test_the_first_refused_dimension_comes_from_the_lds_check(capsys):
    d = hc.first_refused_ndim()
    size = hc.walk_lds(1, d, False)[0]
    _print(capsys, f"walk refusal: ndim {d} (walk_lds_bytes at one slot {size} > 65536; {d - 1}: {hc.walk_lds(1, d - 1, False)[0]}); PB D > 1024 alone would give 1025")
    assert 129 < d < 1025 and size > 64 * 1024 and hc.walk_lds(1, d - 1, False)[0] <= 64 * 1024
