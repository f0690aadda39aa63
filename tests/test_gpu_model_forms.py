"""GPU: the curve and the residual kernels (keprv_kernel, residual_kernel: GpuRVModel.kep_rv_batch / modelk_batch /
residuals_batch, and pointwise.unit_loglik on top of them) against the reference on every model form the golden log-L rows cover
— every parametrisation, a free epoch, the eccentricity clamp, drift orders 1 to 4 with each tref rule, one to three
instruments, two linear series, the no-jitter switch.  Both kernels decode the model on their own, apart from the log-L tile that
tests/test_gpu_loglike.py holds to the same rows; everything computed from merged runs reads them and not the tile.

  a  curves against tests/golden/keprv_edges.npz (the reference's kep_rv and modelk) within golden.curve_bound, a derived bound
     that tests/test_oracle_golden.py shows the reference route itself to stay inside;
  b  the launch: element by element the bits of the full call at sizes below, at and across a workgroup; scalars; exclude_planet;
  c  residuals against tests/golden/residuals_edges.npz by check_residuals' rule, variances bit for bit, keep_planet;
  d  log-L rebuilt by the reference's formula from the device's residuals, and the row sums of pointwise.unit_loglik, against
     the 1506 golden log-L rows: 1e-10 on rows the oracle does not flag RVLL_FLAG_WANDERED, 1e-9 on those it does;
  e  that route against the tile on 512 random rows of six models.

Measured on an MI355X (profiles/r05_model_forms_parity.txt holds every case): of the 1506 rows the oracle flags 189, and none of
them lands between 1e-10 and 1e-9, on the residual route or on the tile; the largest relative error of either is 2.8e-11, on the
eccentricity sweep, and below 2e-15 on every case but the two sweeps.  Curves and residuals reach 1e-4 of their bounds but at the
far times of logk1_logperiod_ml0: 0.11 of the bound (the oracle: 0.076).

Excluding the only planet of a one-planet model gives zeros, for an invalid orbit too: the reference's kep_rv never calls modelk
for the excluded planet (rvmodel:371-380), and the fixture holds its zeros."""
import numpy as np
import pytest

import golden
from evidence_amd import FLAG_INVALID_ORBIT, FLAG_WANDERED, GpuRVModel, pointwise
from test_periodogram_host import check_kept, check_residuals

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]
TOL, TOL_WANDERED = 1e-10, 1e-9          # tests/test_gpu_loglike.py: the parity bar, and the bar of rows with a wandering solve

CURVES = golden.keprv_edge_cases()
RESIDUALS = golden.residual_edge_cases()
LOGLIKE = golden.all_loglike_cases()


def _model(case):
    return GpuRVModel(case.fixed, case.table, case.parnames, linpar_dict=case.linpar or None)


def _curve(m, key, theta, times):
    if key.startswith("pl"):
        return m.modelk_batch(theta, times, planet=int(key[2:]))
    return m.kep_rv_batch(theta, times, exclude_planet=None if key == "exNone" else int(key[2:]))


# ---- a: curves on every form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", CURVES, ids=[cc.name for cc in CURVES])
def test_curves_match_the_reference_on_every_model_form(gpu_required, cc):
    with _model(cc.case) as m:
        assert m.nplanets == cc.nplanets
        got = {key: _curve(m, key, cc.theta, cc.times) for key in cc.curves}
    worst = {key: golden.check_curves(cc, key, got[key]) for key in cc.curves}      # NaN rows as the fixture's, for every mask
    print(f"MODEL_FORMS a {cc.name}: largest |device - reference| over its bound {max(worst.values()):.3e}")


# ---- b: the launch ---------------------------------------------------------------------------------------------------------------
def test_every_element_has_the_bits_of_the_full_call_at_any_launch_size(gpu_required):
    cc = [c for c in CURVES if c.name == "two_planets_two_inst"][0]
    assert cc.nplanets == 2 and len(cc.case.table.insts) == 2 and cc.theta.shape[0] == 6 and cc.times.shape[0] == 41
    times = np.concatenate([cc.times, cc.times[:2]])
    with _model(cc.case) as m:
        for key in ("exNone", "ex1", "ex2", "pl1", "pl2"):
            full = _curve(m, key, cc.theta, times)
            assert np.array_equal(full[:, :41].view(np.uint64), _curve(m, key, cc.theta, cc.times).view(np.uint64))
            golden.check_curves(cc, key, full[:, :41])
            assert np.array_equal(full[:, 41:], full[:, :2])
            for B, Nt in ((1, 1), (1, 41), (6, 1), (5, 41), (6, 43)):               # 1, 41, 6, 205 and 258 threads' worth
                part = _curve(m, key, cc.theta[:B], times[:Nt])
                assert part.shape == (B, Nt) and np.array_equal(part.view(np.uint64), full[:B, :Nt].view(np.uint64)), (key, B, Nt)
        full = m.kep_rv_batch(cc.theta, cc.times)
        one = m.kep_rv_batch(cc.theta[2], float(cc.times[7]))                       # a single vector at a scalar time
        assert one.shape == (1, 1) and one[0, 0] == full[2, 7]
        assert np.array_equal(m.modelk_batch(cc.theta[2], float(cc.times[7]), 2), m.modelk_batch(cc.theta[2:3], cc.times[7:8], 2))
        for nobody in (0, 7):                                                       # rvmodel:373, i != exclude_planet
            assert np.array_equal(m.kep_rv_batch(cc.theta, cc.times, exclude_planet=nobody), full)


def test_excluding_the_only_planet_gives_what_the_reference_gives(gpu_required):
    by_name = {c.name: c for c in CURVES}
    for name in ("direct_ecc_random", "secos_sesin_invalid", "ecos_esin_invalid"):
        cc = by_name[name]
        assert cc.nplanets == 1 and np.isnan(cc.curves["exNone"]).all() == name.endswith("_invalid")
        with _model(cc.case) as m:
            got = m.kep_rv_batch(cc.theta, cc.times, exclude_planet=1)
            whole = m.kep_rv_batch(cc.theta, cc.times)
        assert np.array_equal(got, cc.curves["ex1"]) and np.all(got == 0.0)         # modelk is never called: zeros either way
        assert np.isnan(whole).all() == name.endswith("_invalid")


# ---- c: residuals on every form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case, z", RESIDUALS, ids=[c.name for c, _ in RESIDUALS])
def test_residuals_match_the_reference_on_every_model_form(gpu_required, case, z):
    theta, ref = z[f"{case.name}_theta"], z[f"{case.name}_res"]
    npl = case.layout.nplanets
    with _model(case) as m:
        res, var = m.residuals_batch(theta)
        kept = {p: m.residuals_batch(theta, keep_planet=p) for p in range(1, npl + 1)}
    assert np.array_equal(var, z[f"{case.name}_var"])                               # bit for bit, the no-jitter cases included
    assert np.array_equal(np.isnan(res), np.isnan(ref))
    dead = np.isnan(ref).any(axis=1)
    worst = 0.0
    if not dead.any():
        check_residuals(res, var, z, case)
        scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
        worst = float(np.max(np.abs(res - ref)) / (1e-11 * scale))
    else:
        assert dead.all() and case.name.endswith("_invalid")
    for p, (kres, kvar) in kept.items():
        assert np.array_equal(kvar, var)
        if npl > 1 and not np.isnan(z[f"{case.name}_pl{p}"]).any():
            worst = max(worst, check_kept(kres, z, case, p))
        elif npl == 1:                                                              # nothing is taken out: an invalid orbit's too
            assert np.all(np.isfinite(kres))
            if not dead.any():
                worst = max(worst, check_kept(kres, z, case, p))
    print(f"MODEL_FORMS c {case.name}: largest |device - reference| over its bound {worst:.3e}")


# ---- d: log-L from the device's residuals ------------------------------------------------------------------------------------------
def _held(err, wandered, what):
    """The conditions of a route's relative error against the golden log-L; returns the flagged rows between the two bars."""
    assert err[~wandered].max(initial=0.0) <= TOL, (what, float(err[~wandered].max()), int(np.argmax(np.where(wandered, 0, err))))
    assert err.max() <= TOL_WANDERED, (what, float(err.max()), int(err.argmax()))
    return int(((err > TOL) & wandered).sum())


@pytest.mark.parametrize("case", LOGLIKE, ids=[c.name for c in LOGLIKE])
def test_log_likelihood_rebuilt_from_the_devices_residuals_is_the_references(gpu_required, case):
    from oracle.oracle import OracleModel
    with _model(case) as m:
        res, var = m.residuals_batch(case.theta)
        by_inst = pointwise.unit_loglik(m, case.theta, pointwise.by_instrument(m))
        by_epoch = pointwise.unit_loglik(m, case.theta)
        tile = m.log_likelihood_batch(case.theta)
        layout = m.layout
    _, flags = OracleModel(layout, case.table, case.linpar_series).loglike(case.theta, return_flags=True)
    wandered = (flags & FLAG_WANDERED) != 0
    invalid = case.logL == -1e30
    assert np.array_equal(np.isnan(res).any(axis=1), invalid) and np.array_equal(np.isnan(res).all(axis=1), invalid)
    assert np.all(np.isfinite(var))
    err = golden.rel_err(golden.reference_loglike(res, var), case.logL)
    between = _held(err, wandered, "residuals")
    assert by_inst.shape == (len(invalid), len(case.table.insts)) and by_epoch.shape == res.shape
    assert np.all(by_inst[invalid] == pointwise.INVALID) and np.all(by_epoch[invalid] == pointwise.INVALID)
    assert not np.any(by_inst[~invalid] == pointwise.INVALID) and not np.any(by_epoch[~invalid] == pointwise.INVALID)
    sums = {}
    for name, table in (("by_instrument", by_inst), ("by_epoch", by_epoch)):
        total = np.where(invalid, -1e30, table.sum(axis=1))
        sums[name] = golden.rel_err(total, case.logL)
        _held(sums[name], wandered, name)
    tile_err = golden.rel_err(tile, case.logL)
    print(f"MODEL_FORMS d {case.name}: rows {len(invalid)} invalid {int(invalid.sum())} flagged {int(wandered.sum())}; largest "
          f"relative error: residuals {err.max():.3e}, unit sums {max(s.max() for s in sums.values()):.3e}, tile {tile_err.max():.3e}; "
          f"flagged rows between 1e-10 and 1e-9: residuals {between}, tile {int(((tile_err > TOL) & wandered).sum())}")


# ---- e: the two device routes off the fixtures ---------------------------------------------------------------------------------------
def _route_case(name):
    if name.startswith("cfg"):
        return golden.config_case(int(name[3:]))
    return [c for c in golden.edge_cases() if c.name == name][0]


@pytest.mark.parametrize("name", ["cfg1", "cfg3", "logk1_logperiod_ml0", "secos_sesin_ml0", "three_inst_drift_tref_data",
                                  "linpar_two_series"])
def test_the_tile_and_the_residual_route_agree_on_random_rows(gpu_required, name):
    case = _route_case(name)
    rng = np.random.default_rng(20240)
    theta = rng.uniform(case.theta.min(axis=0), case.theta.max(axis=0), (512, case.theta.shape[1]))
    with _model(case) as m:
        tile, flags = m.log_likelihood_batch(theta, return_flags=True)
        res, var = m.residuals_batch(theta)
    wandered = (flags & FLAG_WANDERED) != 0
    assert np.array_equal((flags & FLAG_INVALID_ORBIT) != 0, np.isnan(res).any(axis=1))
    err = golden.rel_err(golden.reference_loglike(res, var), tile)
    between = _held(err, wandered, name)
    print(f"MODEL_FORMS e {name}: flagged {int(wandered.sum())} of 512; largest relative difference {err.max():.3e}; flagged rows "
          f"between 1e-10 and 1e-9: {between}")
