"""CPU: the oracle (oracle/rvll_oracle.c) against the golden vectors produced by the
reference itself, its Kepler solver against the stored output of the reference's own
compiled solver (and against that build itself when oracle/_ref is present).  This is
what pins the oracle."""
import numpy as np
import pytest

import golden
from oracle import oracle as orc

CASES = golden.all_loglike_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_matches_reference_golden(case):
    om = orc.OracleModel(case.layout, case.table, case.linpar_series)
    got = om.loglike(case.theta)
    err = golden.rel_err(got, case.logL)
    # same libm-level operations as the reference; only numpy's SIMD cos/log kernels differ.  In the eccentricity sweep
    # (239 of 240 rows bit-equal) one row at the 0.99 clamp, where Newton from E = M wanders before it settles, turns that
    # last-bit difference into 2e-12: there the bar is the north star's 1e-10
    tol = 1e-10 if case.name == "high_ecc_sweep" else 5e-13
    assert err.max() <= tol, (case.name, err.max(), int(err.argmax()))
    if case.name == "high_ecc_sweep":
        assert np.count_nonzero(err > 5e-13) <= 2


def test_known_answer_51peg():
    case = golden.peg51_cases()[0]
    om = orc.OracleModel(case.layout, case.table)
    got = om.loglike(case.theta[:1])[0]
    assert abs(got - (-11539.57252446112)) <= 1e-9 * 11539.6          # BASELINE.md known answer


def test_invalid_orbit_sentinel_and_flag():
    for case in CASES:
        if case.name.endswith("_invalid"):
            om = orc.OracleModel(case.layout, case.table)
            got, flags = om.loglike(case.theta, return_flags=True)
            assert np.all(got == -1e30) and np.all(flags & 1)


KEPLER_REF, KEPLER_SAMPLE, KEPLER_ITMAX = golden.kepler_reference()


@pytest.mark.parametrize("ecc", golden.KEPLER_ECCS)
def test_kepler_solver_bit_identical_to_reference_build(ecc):
    M = golden.kepler_mean_anomalies(ecc)
    ref = KEPLER_REF[ecc]                     # the reference's compiled solver on these very M (gen_kepler_golden.py)
    assert golden.sha256(M) == ref["m_sha256"]
    mine, rc1 = orc.trueanomaly(M, ecc)
    assert rc1 == ref["rc"]
    assert np.array_equal(mine[KEPLER_SAMPLE].view(np.uint64), ref["nu_sample"].view(np.uint64))
    assert golden.sha256(mine) == ref["nu_sha256"]
    if orc.load_ref() is not None:            # and against a local build of the reference's solver, when there is one
        live, rc2 = orc.ref_trueanomaly(M, ecc)
        assert rc1 == rc2
        assert np.array_equal(mine, live)


def test_itmax_abort_leaves_tail_untouched_like_reference():
    # an unreachable tolerance forces the niteration >= itmax return (trueanomaly.c:32-33)
    M = golden.kepler_itmax_mean_anomalies()
    mine, rc1 = orc.trueanomaly(M, 0.5, itmax=7, tol=0.0)
    ref, rc2 = KEPLER_ITMAX
    assert rc1 == rc2 == -1
    # elements before the first non-converging one are solved, everything after stays 0 (pre-zeroed nu)
    assert np.array_equal(mine, ref)
    first_zero = int(np.argmax(mine == 0.0))
    assert 0 < first_zero < len(M) and np.all(mine[first_zero:] == 0.0) and np.all(mine[:first_zero] != 0.0)
    if orc.load_ref() is not None:
        live, rc3 = orc.ref_trueanomaly(M, 0.5, itmax=7, tol=0.0)
        assert rc3 == -1 and np.array_equal(mine, live)


def test_iteration_counts_match_survey():
    # e=0 -> 1 step; e=0.3 -> 2-3 steps
    M = np.random.default_rng(3).uniform(-7.0e3, 7.0e3, 5000)
    _, _, it0 = orc.trueanomaly(M, 0.0, want_iters=True)
    _, _, it3 = orc.trueanomaly(M, 0.3, want_iters=True)
    assert it0.min() == it0.max() == 1
    assert it3.min() >= 1 and it3.max() == 3 and 2.8 < it3.mean() < 2.95          # survey: mean 2.87


def test_openmp_batch_equals_serial():
    case = golden.config_case(3)
    om = orc.OracleModel(case.layout, case.table)
    a = om.loglike(case.theta, nthreads=1)
    b = om.loglike(case.theta, nthreads=4)
    assert np.array_equal(a, b)


def test_the_references_value_is_conditioned_worse_than_the_bar_near_the_clamp():
    """OracleModel.conditioning: log-L of the eccentricity sweep with every sin / cos of the Newton loop nudged by one
    unit in the last place.  Up to e = 0.965 nothing moves beyond 1e-13; from 0.975 on individual rows move by 1e-11 ..
    1e-9 — Newton from E = M wanders there before it settles, and where it stops depends on the last bit of libm.  This is
    what "parity with the reference" can mean in that corner (tests/test_gpu_loglike.py)."""
    case = golden.high_ecc_case()
    z = np.load(golden.GOLDEN / "loglike_high_ecc.npz")
    ecc = z["ecc_of_row"]
    om = orc.OracleModel(case.layout, case.table)
    cond = np.maximum(om.conditioning(case.theta, eps=-2.0 ** -53), om.conditioning(case.theta, eps=2.0 ** -52))
    assert cond[ecc <= 0.965].max() <= 1e-13
    assert 1e-11 <= cond[ecc >= 0.975].max() <= 5e-9
    assert np.array_equal(om.loglike(case.theta), om.loglike(case.theta))          # and the probe leaves no trace


def _oracle_curves(layout, table, theta, times, nplanets, keys):
    om = orc.OracleModel(layout, table)
    return {key: om.kep_rv(theta, times, golden.curve_mask(nplanets, key)) for key in keys}


def test_oracle_curves_match_the_references_on_the_configurations():
    """OracleModel.kep_rv, the reference of the host and device tests of everything built on curves, against keprv.npz."""
    import json
    from evidence_amd.layout import compile_layout
    from evidence_amd.synthetic import make_workload
    z = np.load(golden.GOLDEN / "keprv.npz")
    for meta in json.loads((golden.GOLDEN / "keprv.json").read_text()):
        cfg = meta["cfg"]
        w = make_workload(cfg)
        layout = compile_layout(list(w.parnames), dict(w.fixedpardict), w.table.insts, [])
        got = _oracle_curves(layout, w.table, z[f"cfg{cfg}_theta"], z[f"cfg{cfg}_times"], meta["nplanets"], meta["keys"])
        for key in meta["keys"]:
            ref = z[f"cfg{cfg}_{key}"]
            err = float(np.max(np.abs(got[key] - ref)))
            print(f"cfg{cfg} {key}: largest |oracle - reference| {err:.3e}")
            assert got[key].shape == ref.shape and err <= 1e-13 * max(1.0, np.abs(ref).max()), (cfg, key, err)


KEPRV_EDGES = golden.keprv_edge_cases()


def test_the_curve_fixture_covers_every_edge_case_with_a_planet():
    want = [c.name for c in golden.edge_cases() if c.layout.nplanets >= 1]
    assert [cc.name for cc in KEPRV_EDGES] == want and len(want) == 34
    for cc in KEPRV_EDGES:
        t = cc.case.table.time
        assert cc.theta.shape[0] == min(6, cc.case.theta.shape[0]) and np.array_equal(cc.theta, cc.case.theta[:6])
        assert np.array_equal(cc.times[:41], np.linspace(t.min() - 400.3, t.max() + 777.7, 41)) and not np.isin(cc.times, t).any()
        assert cc.far == (cc.name in ("logk1_logperiod_ml0", "secos_sesin_ml0", "free_epoch"))
        assert np.array_equal(cc.times[41:], [t.min() - 1e5, t.max() + 1e5] if cc.far else [])
        assert sorted(cc.curves) == sorted(["exNone"] + [f"{k}{p}" for k in ("ex", "pl") for p in range(1, cc.nplanets + 1)])
        epoch = golden.decode_planets(cc.case, cc.theta)["epoch"]
        assert cc.times.min() < epoch.min()                                # negative phases


@pytest.mark.parametrize("cc", KEPRV_EDGES, ids=[cc.name for cc in KEPRV_EDGES])
def test_oracle_curves_match_the_references_on_every_model_form(cc):
    """... against keprv_edges.npz within golden.curve_bound, the bound the device is held to (tests/test_gpu_model_forms.py):
    the reference route itself stays inside it at every point; NaN rows where the reference returned None."""
    got = _oracle_curves(cc.case.layout, cc.case.table, cc.theta, cc.times, cc.nplanets, cc.curves)
    worst = {key: golden.check_curves(cc, key, got[key]) for key in cc.curves}
    print(cc.name, "largest |oracle - reference| over its bound:", worst)
    invalid = cc.name.endswith("_invalid")
    assert golden.decode_planets(cc.case, cc.theta)["valid"].all() != invalid
    for key, ref in cc.curves.items():
        included = golden.curve_mask(cc.nplanets, key) != 0
        assert np.isnan(ref).all() == (invalid and included) and np.isnan(ref).any() == (invalid and included), key
        if not included:                                                   # kep_rv without its only planet: zeros, valid orbit or not
            assert np.all(ref == 0.0) and np.all(got[key] == 0.0)
