"""The device proposal walk against a plain reference of the same operation, move by move (tests/walk_replay.py).

Move m of a walker draws from (seed, walker, m, .) only, so the walk with nsteps = n is a prefix of the walk with nsteps = N:
launching the device walk from one start with nsteps = 0 .. N gives the device's state after EVERY move, and each single move
n - 1 -> n is replayed on the host, in longdouble, from the device's own state after move n - 1 (walk_replay.check_prefixes: end
rows within TOL_U of the reference, walkers the reference leaves in place bit-identical, theta / log-L those of
prior_loglike_batch at the end row, the launch totals' differences equal to the reference's calls exactly).  No error
accumulates over moves and every decision is judged on its own; only (walker, move) pairs whose decisions the reference itself
marks as within rounding of flipping (fragile: walk_replay's docstring) are left out, at most 0.5 % of a case.

Numbers (profiles/walk_replay.txt).  An end row is compared within TOL_U * scale, scale >= 1 the move's own conditioning figure
from the reference (walk_replay's docstring), never more loosely than TOL_CEILING = 1e-8 (a pair beyond is left out and counts
under the 0.5 % cap).  TOL_U = 2 SPREAD = 7e-13, SPREAD = 3.5e-13 the largest float64 - longdouble distance / scale over the cases
of test_walk_replay_host.py (walk_replay.py says why the margin is 2).  So the bound on a cube coordinate is under 1e-12 for
chord moves (scale 1) and for well-conditioned stepout moves only; measured on the device, the largest scale compared and the
largest error as it is are in the profile, per case.  The errors this file exists for — a wrong bracket end, a counter of the
wrong move, a basis vector from the wrong normals — are of order 1e-3 and more.
"""
import numpy as np
import pytest

import walk_replay as wr
from evidence_amd.callbacks import wrapped_params
from test_gpu_stepout import _model, _start

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
PROPOSALS = ["chord", "stepout"]


def _replay(m, start, wrapped, nsteps, *, proposal, seed=7, walker_base=0, max_rounds=200, step_width=1.0, chol=None, label=""):
    """Device prefixes nsteps = 0 .. N of slice_walk from `start` (_start's tuple), checked move by move; returns the figures."""
    cube, theta, logl, lstar, chol0 = start
    chol = chol0 if chol is None else chol
    states, ncalls = [], []
    for n in range(nsteps + 1):
        c, t, l, used = m.slice_walk(cube, theta, logl, lstar, chol, wrapped, nsteps=n, max_rounds=max_rounds, seed=seed,
                                     walker_base=walker_base, proposal=proposal, step_width=step_width)
        states.append((c, t, l))
        ncalls.append(used)
    assert np.array_equal(states[0][0], cube) and np.array_equal(states[0][2], logl)
    fig = wr.check_prefixes(states, ncalls, m.prior_loglike_batch, tol_u=wr.TOL_U, wrapped=wrapped, proposal=proposal,
                            seed=seed & (2 ** 64 - 1), wid=np.arange(len(cube), dtype=np.uint64) + np.uint64(walker_base), lstar=lstar,
                            chol=chol, max_rounds=max_rounds, step_width=step_width)
    _report(label, proposal, len(cube), nsteps, fig)
    return fig


def _report(label, proposal, k, nsteps, fig):
    print(f"walk replay {label:28s} {proposal:8s} K {k:5d} N {nsteps:3d} pairs {fig.pairs:7d} fragile {fig.fragile:3d} loose {fig.loose:3d} "
          f"exact moves {fig.exact_moves:3d} worst/scale {fig.worst:.2e} worst {fig.worst_abs:.2e} max scale {fig.max_scale:8.1f} "
          f"spread/scale {fig.spread:.2e}")


@pytest.mark.parametrize("proposal", PROPOSALS)
@pytest.mark.parametrize("cfg, k, quantile", [(3, 3000, 0.5), (3, 15000, 0.9), (1, 3000, 0.5), (1, 15000, 0.9)])
def test_every_move_of_the_ordinary_walk(gpu_required, cfg, k, quantile, proposal):
    """K ~ 1500 walkers, N = 2 ndim + 2 moves: a stepout walk crosses two redraws of its basis (m = D - 1 -> D)."""
    with _model(cfg) as m:
        _replay(m, _start(m, k, seed=cfg, quantile=quantile), wrapped_params(m.parnames), 2 * m.ndim + 2, proposal=proposal,
                label=f"cfg{cfg} q{quantile}")


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_without_a_constraint_no_move_is_left_out(gpu_required, proposal):
    with _model(1) as m:
        cube, theta, logl, _, chol = _start(m, 1500, seed=3, quantile=0.0)
        fig = _replay(m, (cube, theta, logl, -np.inf, chol), wrapped_params(m.parnames), 2 * m.ndim + 2, proposal=proposal,
                      label="lstar -inf")
    assert fig.fragile == 0 and fig.exact_moves == 2 * 6 + 2


@pytest.mark.parametrize("proposal", PROPOSALS)
@pytest.mark.parametrize("max_rounds", [1, 2, 5])
def test_moves_given_up_after_max_rounds(gpu_required, max_rounds, proposal):
    """The give-up path and the round counting (stepout: the expansions count against max_rounds too)."""
    with _model(3) as m:
        _replay(m, _start(m, 15000, seed=9, quantile=0.9), wrapped_params(m.parnames), 6, proposal=proposal, max_rounds=max_rounds,
                label=f"max_rounds {max_rounds}")


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_starts_on_the_walls(gpu_required, proposal):
    """u_k = 0 and u_k = nextafter(1, 0) in an unwrapped and in a wrapped coordinate: (0 - u) / d, the clamp, floor."""
    with _model(1) as m:
        wrapped = wrapped_params(m.parnames)
        cube, theta, logl, lstar, chol = _start(m, 4000, seed=5)
        flat, circ = int(np.flatnonzero(~wrapped)[1]), int(np.flatnonzero(wrapped)[0])
        cube = cube.copy()
        cube[0::4, flat], cube[1::4, flat], cube[2::4, circ], cube[3::4, circ] = 0.0, wr.ONE_BELOW, 0.0, wr.ONE_BELOW
        theta, logl = m.prior_loglike_batch(cube)
        keep = logl > lstar
        assert keep.sum() > 200
        _replay(m, (cube[keep], theta[keep], logl[keep], lstar, chol), wrapped, 8, proposal=proposal, label="walls")


@pytest.mark.parametrize("proposal", PROPOSALS)
@pytest.mark.parametrize("shape", ["zero row", "x 1e-6", "x 50"])
def test_degenerate_whitening_factors(gpu_required, shape, proposal):
    """A factor with a zero row (d_k == 0: no limit from that coordinate); a tiny and a huge factor (stepout: brackets wholly
    inside / wholly clamped by the walls — the walk starts in its shrink phase and the ends cost nothing)."""
    with _model(1) as m:
        st = _start(m, 3000, seed=6)
        chol = st[4].copy()
        if shape == "zero row":
            chol[int(np.flatnonzero(~wrapped_params(m.parnames))[0]), :] = 0.0
        else:
            chol *= 1e-6 if shape == "x 1e-6" else 50.0
        _replay(m, st, wrapped_params(m.parnames), 8, proposal=proposal, chol=chol, label=f"chol {shape}")


@pytest.mark.parametrize("step_width", [0.05, 1.0, 20.0])
def test_stepout_bracket_widths(gpu_required, step_width):
    """Many expansions / none."""
    with _model(1) as m:
        _replay(m, _start(m, 3000, seed=8), wrapped_params(m.parnames), 8, proposal="stepout", step_width=step_width,
                max_rounds=1000, label=f"step_width {step_width}")


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_the_high_bits_of_the_counter(gpu_required, proposal):
    with _model(1) as m:
        st = _start(m, 2000, seed=10)
        _replay(m, st, wrapped_params(m.parnames), 8, proposal=proposal, seed=2 ** 64 - 3, walker_base=2 ** 32 - len(st[0]) - 1,
                label="high counters")


@pytest.mark.parametrize("proposal", PROPOSALS)
@pytest.mark.parametrize("k", [1, 7, 9, 3000])
def test_ragged_workgroups(gpu_required, k, proposal):
    """Eight walker slots a workgroup: one walker, one slot short, one over, and 375 workgroups."""
    with _model(1) as m:
        m.set_points_per_block(8)
        cube, theta, logl, lstar, chol = _start(m, 8000, seed=12)
        st = (cube[:k], theta[:k], logl[:k], lstar, chol)
        fig = _replay(m, st, wrapped_params(m.parnames), 8, proposal=proposal, label=f"PB 8, K {k}")
    assert fig.pairs == 8 * k


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_the_queue_refilled_slots_and_the_two_part_launch(gpu_required, proposal, monkeypatch):
    """RVLL_WALK_QUEUE=1 launches as many workgroups as ONE compute unit holds (walk_core; the switch test_gpu_walk.py and
    test_gpu_stepout.py use): at eight walker slots a workgroup and at most 16 workgroups of 256 threads on a compute unit
    that is at most 128 slots for 3000 walkers, so all but the first few come in through the ticket counter into slots
    other walkers have left — a refilled stepout slot has to drop the basis it holds and build the new walker's.  With more
    walkers than slots and nsteps >= 8 walk_core also launches in two parts (the first nsteps / 4 moves, then the rest from
    step_start, most expensive rows first): prefixes n = 8 .. 11 are such launches, and their second part enters a stepout
    basis (D = 6) in the middle, at move 2."""
    monkeypatch.setenv("RVLL_WALK_QUEUE", "1")
    monkeypatch.delenv("RVLL_WALK_PARTS", raising=False)
    with _model(1) as m:
        m.set_points_per_block(8)
        cube, theta, logl, lstar, chol = _start(m, 8000, seed=12)
        st = (cube[:3000], theta[:3000], logl[:3000], lstar, chol)
        fig = _replay(m, st, wrapped_params(m.parnames), 11, proposal=proposal, label="queue 1 CU, PB 8, K 3000")
    assert fig.pairs == 11 * 3000


def test_stepout_refuses_more_than_64_parameters(gpu_required):
    """The stepout normals of 64 parameters use the draws below the shrink draws up exactly (test_walk_replay_host.py); the
    library refuses a stepout walk with more before it launches anything (walk_core: RVLL_E_UNSUPPORTED).  33 instruments with
    an offset and a jitter each: 66 parameters."""
    from evidence_amd import GpuRVModel, RvllError
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    names = [f"i{j:02d}" for j in range(33)]
    table = EpochTable.from_arrays(names, np.arange(66.0), np.zeros(66), np.ones(66), np.repeat(np.arange(33), 2).astype(np.int32))
    pri = {}
    for n in names:
        pri[f"{n}_offset"] = P.Uniform(-10, 10)
        pri[f"{n}_jitter"] = P.Uniform(0, 5)
    with GpuRVModel({}, table, list(pri), priordict=pri) as m:
        assert m.ndim == 66
        cube = np.full((4, 66), 0.5)
        with pytest.raises(RvllError):
            m.slice_walk(cube, cube.copy(), np.zeros(4), -1.0, 0.1 * np.eye(66), None, nsteps=2, seed=1, proposal="stepout")


def test_the_rounds_form(gpu_required):
    with _model(3) as m:
        st = _start(m, 16384, seed=13)
        assert len(st[0]) == 8192
        _replay(m, st, wrapped_params(m.parnames), 3, proposal="chord", label="rounds form")
        assert m.slice_walk_rounds() > 0


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_run_mode_with_every_run_its_own_arguments(gpu_required, proposal):
    """slice_walk_runs: four runs of unequal size, each with its own lstar, factor, seed and number of moves; a row's walker id
    is its index inside its run, and ncalls is per run."""
    with _model(1) as m:
        cube, theta, logl, lstar, chol = _start(m, 3000, seed=14)
        wrapped = wrapped_params(m.parnames)
        k = len(cube)
        run_start = np.array([0, 5, k // 3, k // 3 + 130, k], dtype=np.int64)
        sizes = np.diff(run_start)
        groups = np.repeat(np.arange(4), sizes)
        lst = np.array([lstar, lstar - 1.0, lstar - 0.25, lstar - 3.0])
        chols = np.stack([chol, 0.5 * chol, 2.0 * chol, 0.1 * chol])
        seeds = np.array([3, 2 ** 64 - 1, 5, 2 ** 63], dtype=np.uint64)
        steps = np.array([8, 3, 5, 6])
        states, ncalls = [], []
        for n in range(steps.max() + 1):
            c, t, l, used = m.slice_walk_runs(cube, theta, logl, run_start, lst, chols, wrapped, nsteps=np.minimum(steps, n),
                                              seeds=[int(s) for s in seeds], proposal=proposal, step_width=0.8)
            states.append((c, t, l))
            ncalls.append(used)
        fig = wr.check_prefixes(states, ncalls, m.prior_loglike_batch, tol_u=wr.TOL_U, wrapped=wrapped, groups=groups, steps=steps,
                                proposal=proposal, seed=seeds[groups], wid=np.concatenate([np.arange(s) for s in sizes]),
                                lstar=lst[groups], chol=chols[groups], max_rounds=200, step_width=0.8)
    _report("run mode", proposal, k, int(steps.max()), fig)
    assert fig.pairs == int(np.sum(sizes * steps))


@pytest.mark.parametrize("proposal", PROPOSALS)
def test_the_resident_live_step(gpu_required, proposal):
    """live_step on a resident live set of 400 with the factor supplied, kdead = 50: the rows that replace the dying rows
    order[:kdead] are the replay of the rows `start`, walker i (the one that replaces row order[i]) drawing as walker
    walker_base + i (rvll_live_step, in csrc/rvll_live_host.hip, gathers the start rows into walk rows 0 .. kdead - 1 and hands
    them to walk_core with that base; the end rows are scattered to order[:kdead] in the same order)."""
    with _model(1) as m:
        wrapped = wrapped_params(m.parnames)
        rng = np.random.default_rng(15)
        cube = rng.random((400, m.ndim))
        nsteps, kdead, base, seed = 6, 50, 1000, 99
        states, ncalls = None, [0]
        pick = rng.integers(0, 400 - kdead, kdead)
        for n in range(1, nsteps + 1):
            logl = m.live_init(cube)                          # (the same live set before every prefix)
            order = np.argsort(logl, kind="stable").astype(np.int32)
            lstar = float(logl[order[kdead - 1]])
            start = order[kdead:][pick]
            u0, t0, l0 = m.live_get()
            alive = u0[order[kdead:]]
            d0 = alive - alive.mean(axis=0)
            chol = np.linalg.cholesky(d0.T @ d0 / (len(alive) - 1) + 1e-14 * np.eye(m.ndim))
            if states is None:
                states = [(u0[start], t0[start], l0[start])]
            new_l, used = m.live_step(order, kdead, start, lstar, wrapped, nsteps=n, seed=seed, walker_base=base, chol=chol,
                                      proposal=proposal, step_width=1.0)
            u1, t1, l1 = m.live_get()
            assert np.array_equal(l1[order[:kdead]], new_l)
            rest = order[kdead:]
            assert np.array_equal(u1[rest], u0[rest]) and np.array_equal(l1[rest], l0[rest])        # the survivors stay
            states.append((u1[order[:kdead]], t1[order[:kdead]], l1[order[:kdead]]))
            ncalls.append(used)
        fig = wr.check_prefixes(states, ncalls, m.prior_loglike_batch, tol_u=wr.TOL_U, wrapped=wrapped, proposal=proposal, seed=seed,
                                wid=np.arange(kdead) + base, lstar=lstar, chol=chol, max_rounds=200, step_width=1.0)
    _report("live_step", proposal, kdead, nsteps, fig)
    assert fig.pairs == nsteps * kdead
