"""CPU: tests/reduced_cases.py on the oracle alone — is the float32 emulation of the reduced-precision modes in the modes' own
error class, and are its cases what tests/test_gpu_reduced_shapes.py needs (finite, nothing wandering, no solve handed to the
double solver unless the case is about that, marks a float solver can be held to)?  Prints the yardsticks
Y[case, precision, tol, itmax] the GPU file bounds the device by, and the calibration table (run with -s to see them)."""
from types import SimpleNamespace

import numpy as np
import pytest

import reduced_cases as rc
import solver_cases as sc
from evidence_amd import FLAG_NONCONVERGED, FLAG_WANDERED
from evidence_amd.synthetic import make_workload

# the device's maxima against its own fp64 path on the samples of test_tolerance_sweep, as recorded in the comment above BOUNDS
# in tests/test_gpu_precision.py (cfg -> mixed, fp32)
DEVICE_RECORD = {2: (1.03e-7, 9.93e-8), 3: (1.72e-7, 1.85e-7), 5: (6.57e-8, 6.38e-8)}
SWEEP = {2: 4096, 3: 8192, 5: 1024}                    # test_tolerance_sweep's sizes; its seeds are 321 + cfg


def sweep_case(cfg):
    w = make_workload(cfg)
    return SimpleNamespace(name=f"cfg{cfg}", table=w.table, parnames=list(w.parnames), fixed=dict(w.fixedpardict),
                           theta=w.sample_theta(SWEEP[cfg], seed=321 + cfg), linpar={}, nplanets=sum("k1" in n for n in w.parnames))


@pytest.mark.parametrize("cfg", sorted(SWEEP))
def test_the_emulation_is_in_the_modes_error_class(cfg):
    """On the very samples of test_tolerance_sweep the emulation is at least a quarter as far from the fp64 oracle as the device
    was recorded to be from its fp64 path: four times the emulation's distance does not fail the device as it is known."""
    case = sweep_case(cfg)
    for precision, record in zip(rc.PRECISIONS, DEVICE_RECORD[cfg]):
        y = rc.yardstick(case, precision)
        print(f"calibration cfg{cfg} {precision}: emulation max {y.max:.3e} median {y.median:.3e} | device record max {record:.3e} "
              f"| device / emulation {record / y.max:.2f}")
        assert y.handed == 0
        assert y.max >= 0.25 * record, (cfg, precision, y.max, record)


RUNS = rc.runs()


@pytest.mark.parametrize("case, tol, itmax", RUNS, ids=[rc.run_id(*r) for r in RUNS])
def test_cases_are_what_the_gpu_tests_need(case, tol, itmax):
    ref, rflags = rc.oracle_of(case, tol, itmax)
    assert np.isfinite(ref).all() and case.theta.shape[0] >= 256
    assert not (rflags & FLAG_WANDERED).any() and not rflags.any()
    # at the case's own geometry (256 CUs for the CU-wide form): which items of the pair path stop together
    geometry = (case.form, case.pb if case.form == "tile" else rc.cu_geometry(case.theta.shape[0], case.n_epochs)[0])
    for precision in rc.PRECISIONS:
        y = rc.yardstick(case, precision, tol, itmax, geometry)
        print(f"Y[{rc.run_id(case, tol, itmax)}, {precision}, {geometry[0]} x {geometry[1]}] = {y.max:.3e} (median {y.median:.3e}, handed over {y.handed} of {y.items})")
        if tol < rc.F32_MIN_TOL:
            # no float step can show such a tol met: every solve is the double solver's, and the emulation is the oracle's
            # arithmetic up to the float chi-square of fp32
            assert y.handed == y.items
            if precision == "mixed":
                assert y.max <= 1e-12, y.max
        else:
            assert y.handed == 0
        assert np.isfinite(y.max) and (y.max > 0 or case.nplanets == 0)


def test_the_case_list_covers_what_it_claims():
    """Items per 256-thread tile, LDS windows, planet counts, instruments, drift and linear terms, both item paths, tol."""
    cases = rc.cases()
    tile = {c.n_epochs * c.pb for c in cases if c.form == "tile"}
    assert {1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 1000} <= tile
    assert {(4097, 1), (4097, 2), (4500, 1), (4500, 2), (8492, 1), (8492, 2)} <= {(c.n_epochs, c.pb) for c in cases}
    assert {0, 1, 2, 3, 5, 8} <= {c.nplanets for c in cases}
    assert max(len(c.table.insts) for c in cases) == 5
    assert {0, 1, 3} <= {len(c.linpar) for c in cases}
    assert {True, False} <= {any("drift" in n for n in c.parnames) for c in cases}
    single = {c.n_epochs * max(c.pb, 1) for c in cases if (1e-4, 16) in c.runs and c.form == "tile"}
    assert {63, 64, 65, 257, 300, 1000} <= single and any(c.n_epochs == 4500 and (1e-4, 16) in c.runs for c in cases)
    assert sum((1e-2, 10000) in c.runs for c in cases) == 3 and sum((1e-9, 10000) in c.runs for c in cases) == 3
    # the CU-wide form on 256 CUs: one, two, an odd and an even number of rounds from three and four on, full and ragged each
    geo = {rc.cu_geometry(c.theta.shape[0], c.n_epochs)[1:] for c in cases if c.form == "cu"}
    kinds = {(1 if r == 1 else 2 if r == 2 else "odd" if r % 2 else "even", ragged) for r, ragged in geo}
    assert kinds == {(k, g) for k in (1, 2, "odd", "even") for g in (False, True)}, kinds
    for c in cases:
        if c.wraps:
            pb = rc.cu_geometry(c.theta.shape[0], c.n_epochs)[0]
            assert (rc.wrap_start_rounds(c, pb) > 0).sum() >= 32, c.name          # tiles that start past round 0, and wrap


def test_the_handover_solver_is_the_references_rule():
    rng = np.random.default_rng(4)
    M, ecc = rng.uniform(-40, 40, 4000), rng.uniform(0, 0.95, 4000)
    for tol, cap in ((1e-4, 10000), (1e-9, 10000), (1e-4, 5)):
        assert np.array_equal(rc.newton_f64(M, ecc, tol, cap)[1], sc.newton_counts(rc.sincos_numpy, M, ecc, tol, cap))


def test_marks_a_float_solver_can_be_held_to():
    """itmax = 5 on solver_cases.placed(200, 256): on at least three quarters of the rows the first failing epoch of both planets
    is the same for a double and for a float solver, whatever the last bit of the float sin / cos; at least 32 of them carry a
    mark strictly inside the array; and there the emulation's flags are the oracle's."""
    case, keep, inside, plain = rc.placed_rows()
    print(f"placed(200, 256) at itmax 5: {plain} rows agree with numpy's float sin / cos, {int(keep.sum())} also when nudged one "
          f"float ulp either way, {int(inside.sum())} of those with a mark inside the array")
    assert keep.sum() >= 0.75 * keep.size and inside.sum() >= 32
    kept = rc.placed_kept_case()
    for precision in rc.PRECISIONS:
        y = rc.yardstick(kept, precision, 1e-4, sc.PLACED_ITMAX)
        info = {}
        rc.emulate(kept, precision, 1e-4, sc.PLACED_ITMAX, info=info)
        print(f"Y[placed200_kept itmax 5, {precision}] = {y.max:.3e} (median {y.median:.3e})")
        assert np.array_equal(info["flags"], y.rflags & FLAG_NONCONVERGED) and not (y.rflags & ~FLAG_NONCONVERGED).any()
        assert y.handed == 0 and (y.rflags != 0).sum() >= 32
