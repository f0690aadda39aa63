"""The device proposal walk at 48 to 129 parameters, move by move against tests/walk_replay.py (as test_gpu_walk_replay.py does at
6 to 19): both sides of the LDS staging of the whitening factor (kWalkCholLds = 48: from 49 the factor is read from global
memory and every LDS pointer behind it moves), the stepout maximum of 64 (a 64-vector Gram-Schmidt basis on the device, the
normals' top draw field 8191 next to the first shrink draw 8192), walker slots that walk_args had to shrink, the queue and the
two-part launch, the rounds form, run mode and the resident step with the device's own factor — and the dimension walk_args
refuses.  The cases, the model and the LDS arithmetic are tests/highdim_cases.py; tests/test_highdim_cases_host.py shows that
the reference alone meets the comparison's conditions for every case here.  TOL_U, SPREAD and the fragile cap are walk_replay's,
unchanged.  Figures: profiles/highdim_replay.txt."""
import numpy as np
import pytest

import highdim_cases as hc
import walk_replay as wr
from evidence_amd import RvllError, _abi
from test_gpu_stepout import _start
from test_gpu_walk_replay import _replay, _report

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def _case_start(m, c):
    st = _start(m, c.k, seed=c.seed)
    assert len(st[0]) == c.k // 2
    return st


@pytest.mark.parametrize("name", ["D48 chord", "D48 stepout", "D49 chord", "D49 stepout", "D64 chord", "D64 stepout", "D129 chord"])
def test_every_move_on_both_sides_of_the_factor_staging(gpu_required, name):
    """300 walkers, 6 moves, the launch geometry asked for 32 slots a workgroup: walk_args has to shrink them until the LDS fits
    (to highdim_cases.walk_slots: 12, 18, 13 and 6 at 48, 49, 64 and 129 parameters) and widen the tile's window to 3 PB D."""
    c = hc.WALK_CASE[name]
    assert 1 <= hc.walk_slots(c.ndim, c.proposal == "stepout") < 32
    with hc.offsets_model(c.ndim) as m:
        m.set_points_per_block(32)
        fig = _replay(m, _case_start(m, c), hc.wrapped(c.ndim), c.nsteps, proposal=c.proposal, label=f"{name}, PB asked 32")
    assert fig.pairs == c.nsteps * (c.k // 2)


@pytest.mark.parametrize("name", ["D49 chord", "D64 stepout", "D129 chord"])
def test_every_move_with_the_slots_the_library_chooses(gpu_required, name):
    c = hc.WALK_CASE[name]
    with hc.offsets_model(c.ndim) as m:
        fig = _replay(m, _case_start(m, c), hc.wrapped(c.ndim), c.nsteps, proposal=c.proposal, label=f"{name}, default PB")
    assert fig.pairs == c.nsteps * (c.k // 2)


def test_stepout_across_a_basis_redraw_at_64_parameters(gpu_required):
    """32 walkers, 66 moves: every vector of a 64-vector basis is built and used (m = 0 .. 63), the basis is redrawn at m = 64,
    and the last normal's second uniform (draw field 8191) is drawn next to the first shrink draw (8192)."""
    c = hc.WALK_CASE["D64 stepout redraw"]
    with hc.offsets_model(c.ndim) as m:
        fig = _replay(m, _case_start(m, c), hc.wrapped(c.ndim), c.nsteps, proposal="stepout", label=c.name)
    assert fig.pairs == 66 * 32


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_the_queue_and_the_two_part_launch_at_49_parameters(gpu_required, proposal, monkeypatch):
    """RVLL_WALK_QUEUE=1: as many workgroups as one compute unit holds, so most of the 600 walkers come in through the ticket
    counter into slots other walkers have left (a refilled stepout slot drops its 49-vector basis and builds the new walker's);
    prefixes 8 and 9 go in two parts."""
    monkeypatch.setenv("RVLL_WALK_QUEUE", "1")
    monkeypatch.delenv("RVLL_WALK_PARTS", raising=False)
    c = hc.WALK_CASE[f"D49 queue {proposal}"]
    with hc.offsets_model(c.ndim) as m:
        fig = _replay(m, _case_start(m, c), hc.wrapped(c.ndim), c.nsteps, proposal=proposal, label="D49 queue 1 CU")
    assert fig.pairs == 9 * 600


def test_the_rows_form_at_49_parameters(gpu_required, monkeypatch):
    """RVLL_WALK_ROWS=1: the second part of prefixes 8 and 9 (after one move through the queue) runs in slice_walk_rows_kernel,
    whose LDS chain has the same edge — the parked rows [R][D] start behind chol_s, which is empty from D = 49
    (walk_rows_lds_bytes counts what the chain of rvll_walk.hip lines 55 - 93 reaches: 2 PB D + 4 PB + R D + R doubles,
    16 PB + 6 + D + 4 R ints)."""
    monkeypatch.setenv("RVLL_WALK_QUEUE", "1")
    monkeypatch.setenv("RVLL_WALK_ROWS", "1")
    monkeypatch.delenv("RVLL_WALK_PARTS", raising=False)
    c = hc.WALK_CASE["D49 queue chord"]
    with hc.offsets_model(c.ndim) as m:
        fig = _replay(m, _case_start(m, c), hc.wrapped(c.ndim), c.nsteps, proposal="chord", label="D49 rows form, 1 CU")
    assert fig.pairs == 9 * 600


def test_the_rounds_form_at_49_parameters(gpu_required):
    """8192 walkers take the rounds form by default; its step's LDS (rvll_rounds.h step_lds_bytes: 4 W D + 2 W spec + 3 W doubles,
    2 W spec + 8 W + 4 + D ints) holds W = 35 walkers a workgroup within 60 KiB at D = 49, spec = 4, so walk_rounds does not
    refuse and the rounds form is what runs; its direction kernel reads the factor from global memory from D = 49 too."""
    c = hc.WALK_CASE["D49 rounds"]
    step_lds = lambda w: 8 * (4 * w * 49 + 2 * w * 4 + 3 * w) + 4 * (2 * w * 4 + 8 * w + 4 + 49) + 16
    assert step_lds(35) <= 60 * 1024 < step_lds(36)
    with hc.offsets_model(c.ndim) as m:
        st = _case_start(m, c)
        assert len(st[0]) == 8192
        _replay(m, st, hc.wrapped(c.ndim), c.nsteps, proposal="chord", label="D49 rounds form")
        rounds = m.slice_walk_rounds()
    print(f"walk form at D 49, K 8192: {'rounds form, ' + str(rounds) + ' rounds' if rounds else 'single-kernel form'}")
    assert rounds > 0


@pytest.mark.parametrize("proposal", ["chord", "stepout"])
def test_run_mode_at_64_parameters(gpu_required, proposal):
    """slice_walk_runs: four runs of 5, 60, 130 and 100 rows with their own lstar, factor (read from global memory per walker),
    seed and step count."""
    c = hc.RUN_MODE
    with hc.offsets_model(c.ndim) as m:
        cube, theta, logl, lstar, chol = _start(m, c.k, seed=c.seed)
        wrapped = hc.wrapped(c.ndim)
        sizes, steps = np.array(c.sizes), np.array(c.steps)
        assert len(cube) == sizes.sum()
        run_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        groups = np.repeat(np.arange(4), sizes)
        lst, chols, seeds = hc.run_mode_arguments(lstar, chol)
        states, ncalls = [], []
        for n in range(steps.max() + 1):
            u, t, l, used = m.slice_walk_runs(cube, theta, logl, run_start, lst, chols, wrapped, nsteps=np.minimum(steps, n),
                                              seeds=[int(s) for s in seeds], proposal=proposal, step_width=0.8)
            states.append((u, t, l))
            ncalls.append(used)
        fig = wr.check_prefixes(states, ncalls, m.prior_loglike_batch, tol_u=wr.TOL_U, wrapped=wrapped, groups=groups, steps=steps,
                                proposal=proposal, seed=seeds[groups], wid=np.concatenate([np.arange(s) for s in sizes]),
                                lstar=lst[groups], chol=chols[groups], max_rounds=200, step_width=0.8)
    _report("D64 run mode", proposal, len(cube), int(steps.max()), fig)
    assert fig.pairs == int(np.sum(sizes * steps))


@pytest.mark.parametrize("ndim, proposal", [(49, "chord"), (49, "stepout"), (129, "chord")])
def test_the_resident_step_with_the_devices_own_factor(gpu_required, ndim, proposal):
    """live_step on 400 resident rows, kdead = 50, the factor from the survivors' covariance summed on the device (moments_cov's
    global-memory path: D > 45; moments_sum with one row group a block at 129): the end rows are the replay with the factor the
    step returns, the survivors stay bit-identical, and the factor is the longdouble factor of the survivors within the bound
    test_gpu_live_highdim.py uses."""
    c = hc.LIVE_STEP
    with hc.offsets_model(ndim) as m:
        wrapped = hc.wrapped(ndim)
        cube, order, lstar, start = hc.live_step_case(ndim, m.live_init)
        rest = order[c.kdead:]
        states, ncalls, chol = None, [0], None
        for n in range(1, c.nsteps + 1):
            logl = m.live_init(cube)                          # (the same live set before every prefix)
            assert lstar == float(logl[order[c.kdead - 1]])
            u0, t0, l0 = m.live_get()
            if states is None:
                states = [(u0[start], t0[start], l0[start])]
            new_l, used, used_chol = m.live_step(order, c.kdead, start, lstar, wrapped, nsteps=n, seed=c.seed, walker_base=c.base,
                                                 return_chol=True, proposal=proposal, step_width=1.0)
            assert chol is None or np.array_equal(chol, used_chol)
            chol = used_chol
            u1, t1, l1 = m.live_get()
            assert np.array_equal(l1[order[:c.kdead]], new_l)
            assert np.array_equal(u1[rest], u0[rest]) and np.array_equal(t1[rest], t0[rest]) and np.array_equal(l1[rest], l0[rest])
            states.append((u1[order[:c.kdead]], t1[order[:c.kdead]], l1[order[:c.kdead]]))
            ncalls.append(used)
        bound, host, ref = hc.factor_bound(cube[rest])
        dist = hc.factor_distance(chol, ref)
        print(f"live_step factor D {ndim:3d} n {len(rest):4d}: device - longdouble {dist:.2e} of max|L|, bound {bound:.2e} (float64 numpy {host:.2e})")
        assert np.all(np.triu(chol, 1) == 0) and dist <= bound
        fig = wr.check_prefixes(states, ncalls, m.prior_loglike_batch, tol_u=wr.TOL_U, wrapped=wrapped, proposal=proposal, seed=c.seed,
                                wid=np.arange(c.kdead) + c.base, lstar=lstar, chol=chol, max_rounds=200, step_width=1.0)
    _report(f"D{ndim} live_step", proposal, c.kdead, c.nsteps, fig)
    assert fig.pairs == c.nsteps * c.kdead


def test_the_walk_refuses_the_first_dimension_its_lds_cannot_hold(gpu_required):
    """walk_args refuses where walk_lds_bytes at one walker slot passes 64 KiB — before PB D > 1024 could (ndim 1025): the
    dimension is computed from the code's formulas (highdim_cases.first_refused_ndim), not taken from a launch.  Nothing is
    launched, and a walk on an ordinary model works afterwards."""
    d = hc.first_refused_ndim()
    assert 129 < d < 1025
    with hc.offsets_model(d) as m:
        assert m.ndim == d
        cube = np.full((4, d), 0.5)
        with pytest.raises(RvllError) as err:
            m.slice_walk(cube, cube.copy(), np.zeros(4), -1.0, 0.1 * np.eye(d), None, nsteps=2, seed=1)
        assert err.value.code == _abi.E_UNSUPPORTED
    with hc.offsets_model(7) as m:
        fig = _replay(m, _start(m, 400, seed=3), hc.wrapped(7), 3, proposal="chord", label="D7 after the refusal")
    assert fig.pairs == 3 * 200
