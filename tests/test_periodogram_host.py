"""CPU: the numpy definitions of evidence_amd/periodogram.py.  The generalised Lomb-Scargle power against a per-row Python loop,
on an exact sinusoid, under the transformations it is invariant to, and on NaN / degenerate rows; the default grid and the
refusals; the prototypes of the device entries; residuals_definition on the oracle's curves against what the reference's own
log_likelihood lines give for the two shipped 51 Peg configurations (tests/golden/residuals_51peg.npz, made by
gen_residuals_golden.py)."""
import math

import numpy as np
import pytest

import golden
from evidence_amd import _abi, periodogram
from test_predictive_host import OracleCurves


def _series(ne, seed):
    """Epochs on a 2^-10 d raster (so that a shift by a power of two moves them exactly), residuals and variances."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.choice(100 * 1024, size=ne, replace=False)) / 1024.0
    return t, rng.normal(0.0, 5.0, ne), rng.uniform(0.5, 9.0, ne)


def _loop(time, res, var, f0, df, nfreq):
    out, det = np.full((res.shape[0], nfreq), np.nan), np.full((res.shape[0], nfreq), np.nan)
    tmin = min(time)
    for b in range(res.shape[0]):
        if any(math.isnan(x) for x in res[b]) or any(math.isnan(x) for x in var[b]):
            continue
        tot = sum(1.0 / v for v in var[b])
        w = [1.0 / v / tot for v in var[b]]
        for k in range(nfreq):
            f = f0 + df * k
            c = [math.cos(2.0 * math.pi * f * (t - tmin)) for t in time]
            s = [math.sin(2.0 * math.pi * f * (t - tmin)) for t in time]
            r = res[b]
            Y = sum(wi * ri for wi, ri in zip(w, r))
            C = sum(wi * ci for wi, ci in zip(w, c))
            S = sum(wi * si for wi, si in zip(w, s))
            YY = sum(wi * ri * ri for wi, ri in zip(w, r)) - Y * Y
            YC = sum(wi * ri * ci for wi, ri, ci in zip(w, r, c)) - Y * C
            YS = sum(wi * ri * si for wi, ri, si in zip(w, r, s)) - Y * S
            CC = sum(wi * ci * ci for wi, ci in zip(w, c)) - C * C
            SS = sum(wi * si * si for wi, si in zip(w, s)) - S * S
            CS = sum(wi * ci * si for wi, ci, si in zip(w, c, s)) - C * S
            D = CC * SS - CS * CS
            det[b, k] = D
            if YY * D > 0:
                out[b, k] = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / (YY * D)
    return out, det


@pytest.mark.parametrize("ne", [4, 7, 64])
def test_the_definition_matches_a_loop_over_rows_and_frequencies(ne):
    t, _, _ = _series(ne, ne)
    rng = np.random.default_rng(100 + ne)
    res, var = rng.normal(0.0, 5.0, (5, ne)), rng.uniform(0.5, 9.0, (5, ne))
    res[3, 1] = np.nan                                                    # a NaN row
    f0, df, nfreq = 1.0 / 100.0, 1.0 / 800.0, 37
    got = periodogram.gls_definition(t, res, var, f0, df, nfreq)
    want, det = _loop(t, res, var, f0, df, nfreq)
    assert got.shape == (5, 37) and np.array_equal(np.isnan(got), np.isnan(want)) and np.all(np.isnan(got[3]))
    ok = ~np.isnan(want)
    # sums of <= 64 terms of magnitude <= 1 in another order move by a few 1e-16 each, the phases of another order of
    # multiplication by 2 pi f tau 2^-53 <= 4e-15; the quotient amplifies either by 1 / D (D = CC SS - CS^2 <= 1/4)
    cond = 1.0 / np.minimum(det[ok], 1.0)
    assert np.all(det[ok] > 0.0) and np.all(np.abs(got[ok] - want[ok]) <= 1e-14 * cond)
    assert np.all(got[ok] >= 0.0) and np.all(got[ok] <= 1.0 + 1e-12)
    for order in ("ftau", "tau_f"):
        other = periodogram.gls_definition(t, res, var, f0, df, nfreq, phase=order)
        assert np.all(np.abs(other[ok] - got[ok]) <= 1e-13 * cond)
    wide = periodogram.gls_definition(t, res, var, f0, df, nfreq, dtype=np.longdouble)
    assert wide.dtype == np.longdouble and np.all(np.abs(wide[ok] - got[ok]) <= 1e-13 * cond)


@pytest.mark.parametrize("ne", [4, 9, 64])
def test_a_sinusoid_with_an_offset_at_a_grid_frequency_has_power_one(ne):
    t, _, var = _series(ne, 10 + ne)
    f0, df, nfreq = 1.0 / 100.0, 1.0 / 800.0, 64
    for k in (0, 5, 63):
        ph = 2.0 * np.pi * (f0 + df * k) * (t - t.min())
        r = 3.0 * np.cos(ph) - 2.0 * np.sin(ph) + 5.0
        p = periodogram.gls_definition(t, r, var, f0, df, nfreq)
        assert abs(p[0, k] - 1.0) <= 1e-12 and np.nanmax(p) <= 1.0 + 1e-12


def test_the_power_does_not_change_under_a_time_shift_a_constant_or_a_factor_on_the_variances():
    t, r, var = _series(48, 3)
    f0, df, nfreq = 1.0 / 100.0, 1.0 / 800.0, 200
    base = periodogram.gls_definition(t, r, var, f0, df, nfreq)
    assert np.all(np.isfinite(base))
    for moved in (periodogram.gls_definition(t + 4096.0, r, var, f0, df, nfreq),
                  periodogram.gls_definition(t, r + 7.25, var, f0, df, nfreq),
                  periodogram.gls_definition(t, r, 3.7 * var, f0, df, nfreq)):
        assert np.max(np.abs(moved - base)) <= 1e-12


def test_nan_rows_and_degenerate_rows_give_nan():
    t, r, var = _series(12, 4)
    f0, df, nfreq = 0.01, 0.00125, 9
    res = np.stack([r, np.zeros(12), np.where(np.arange(12) == 5, np.nan, r), r])
    vv = np.stack([var, var, var, np.where(np.arange(12) == 0, np.nan, var)])
    p = periodogram.gls_definition(t, res, vv, f0, df, nfreq)
    assert np.all(np.isfinite(p[0])) and np.all(np.isnan(p[1:]))          # YY = 0; NaN residual; NaN variance
    same = periodogram.gls_definition(np.full(12, 50000.0), r, var, f0, df, nfreq)
    assert np.all(np.isnan(same))                                         # every phase 0: SS = CS = 0, so D = 0
    idx, pk = periodogram.peaks_definition(p)
    assert idx.dtype == np.int32 and idx[0] == int(np.argmax(p[0])) and pk[0] == p[0].max()
    assert list(idx[1:]) == [-1, -1, -1] and np.all(np.isnan(pk[1:]))
    mixed = np.array([[0.1, np.nan, 0.9, np.nan], [0.5, 0.7, 0.7, 0.2]])
    idx, pk = periodogram.peaks_definition(mixed)
    assert list(idx) == [1, 1] and np.isnan(pk[0]) and pk[1] == 0.7       # numpy's argmax: the first NaN, the first of equals


def test_the_default_grid():
    t = np.array([3.0, 0.0, 1.0, 10.0, 2.0, 6.0])                         # spacings 1 1 1 3 4: median 1, pmin 2
    f0, df, nfreq = periodogram.frequency_grid(t)
    assert f0 == df == 1.0 / 80.0 and nfreq == 40 and f0 + df * (nfreq - 1) <= 0.5
    assert periodogram.frequency_grid(t, oversample=2, pmin=5.0) == (0.05, 0.05, 4)
    for bad in (dict(time=t[:3]), dict(time=np.zeros(6)), dict(time=t, oversample=0), dict(time=t, pmin=0.0),
                dict(time=t, pmin=np.inf), dict(time=[0.0, 0.0, 0.0, 0.0, 1.0])):
        with pytest.raises(ValueError):
            periodogram.frequency_grid(**bad)


def test_refusals_and_the_prototypes():
    t, r, var = _series(8, 5)
    for bad in (dict(f0=0.0), dict(f0=-1.0), dict(f0=np.nan), dict(df=0.0), dict(df=-0.1), dict(df=np.inf), dict(nfreq=0),
                dict(nfreq=-3), dict(nfreq=2.5), dict(nfreq=(1 << 24) + 1)):
        kw = dict(f0=0.01, df=0.01, nfreq=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            periodogram.gls_definition(t, r, var, **kw)
        with pytest.raises(ValueError):
            periodogram.check_grid(**kw)
    with pytest.raises(ValueError, match="epochs"):
        periodogram.gls_definition(t[:3], r[:3], var[:3], 0.01, 0.01, 4)
    with pytest.raises(ValueError, match="epochs"):
        periodogram.check_grid(0.01, 0.01, 4, nepochs=3)
    with pytest.raises(ValueError):
        periodogram.gls_definition(t, r[:7], var[:7], 0.01, 0.01, 4)
    with pytest.raises(ValueError, match="phase"):
        periodogram.gls_definition(t, r, var, 0.01, 0.01, 4, phase="other")
    assert periodogram.check_grid(0.5, 0.25, 7, nepochs=4) == (0.5, 0.25, 7)
    assert "rvll_residuals_batch" in _abi.PROTOTYPES and "rvll_gls_bands" in _abi.PROTOTYPES
    assert len(_abi.PROTOTYPES["rvll_gls_bands"][1]) == 18 and len(_abi.PROTOTYPES["rvll_residuals_batch"][1]) == 6
    assert _abi.ABI_VERSION == (0, 8)
    lib = _abi.load()
    assert hasattr(lib, "rvll_residuals_batch") and hasattr(lib, "rvll_gls_bands")


def check_residuals(res, var, z, case, rows=slice(None)):
    """(res, var) against the fixture: res to 1e-11 of max(|vrad|, the curve's amplitude) — the bound tests/test_gpu_curves.py
    holds the curves to —, var exactly."""
    scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
    assert res.shape == z[f"{case.name}_res"][rows].shape
    assert np.max(np.abs(res - z[f"{case.name}_res"][rows])) <= 1e-11 * scale
    assert np.array_equal(var, z[f"{case.name}_var"][rows])


@pytest.mark.parametrize("case", golden.peg51_cases(), ids=lambda c: c.name)
def test_residuals_match_the_references_log_likelihood_lines_on_the_oracles_curves(case):
    z = np.load(golden.GOLDEN / "residuals_51peg.npz")
    theta = z[f"{case.name}_theta"]
    assert theta.shape[0] == 2 and theta[1, case.parnames.index("planet1_ecc")] == 0.6
    model = OracleCurves(case)
    res, var = periodogram.residuals_definition(model, theta)
    check_residuals(res, var, z, case)
    one, one_var = periodogram.residuals_definition(model, theta[1])              # a single vector is a batch of one
    assert np.array_equal(one[0], res[1]) and np.array_equal(one_var[0], var[1])
    assert (case.name == "51peg_drift") == case.layout.has_drift
    # keep_planet=1 leaves the planet in: the residuals differ by its curve
    kept, kept_var = periodogram.residuals_definition(model, theta, keep_planet=1)
    scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
    assert np.max(np.abs(kept - (z[f"{case.name}_res"] + z[f"{case.name}_kep"]))) <= 1e-11 * scale
    assert np.array_equal(kept_var, var)
    with pytest.raises(ValueError, match="parameters"):
        periodogram.residuals_definition(model, theta[:, :-1])
    with pytest.raises(AssertionError):
        periodogram.residuals_definition(model, theta, keep_planet=1.0)


RESIDUAL_EDGES = golden.residual_edge_cases()


def check_kept(kept, z, case, p, rows=slice(None)):
    """residuals with keep_planet=p against the fixture's res plus the reference's modelk of planet p at the epochs (the Keplerian
    sum itself where p is the only planet), within check_residuals' bound."""
    ref_p = z[f"{case.name}_pl{p}"] if case.layout.nplanets > 1 else z[f"{case.name}_kep"]
    scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
    err = np.max(np.abs(kept - (z[f"{case.name}_res"] + ref_p)[rows]))
    assert err <= 1e-11 * scale, (case.name, p, float(err))
    return float(err / (1e-11 * scale))


@pytest.mark.parametrize("case, z", RESIDUAL_EDGES, ids=[c.name for c, _ in RESIDUAL_EDGES])
def test_residuals_match_the_references_lines_on_every_model_form(case, z):
    """residuals_definition on the oracle's curves against residuals_edges.npz: every parametrisation, drift order, tref rule,
    instrument count, linear series and the no-jitter switch; an invalid orbit is a NaN row of res beside its var."""
    theta = z[f"{case.name}_theta"]
    assert np.array_equal(theta, case.theta[:3])
    ref = z[f"{case.name}_res"]
    dead = np.isnan(ref).any(axis=1)
    assert np.array_equal(dead, np.isnan(ref).all(axis=1)) and dead.all() == case.name.endswith("_invalid")
    model = OracleCurves(case)
    res, var = periodogram.residuals_definition(model, theta)
    assert np.array_equal(np.isnan(res), np.isnan(ref)) and np.array_equal(var, z[f"{case.name}_var"])
    if not dead.all():
        scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
        print(case.name, "largest |res - reference| over its bound:", float(np.max(np.abs(res - ref)[~dead]) / (1e-11 * scale)))
        check_residuals(res, var, z, case)
    for p in range(1, case.layout.nplanets + 1 if case.layout.nplanets > 1 else 1):
        kept, kept_var = periodogram.residuals_definition(model, theta, keep_planet=p)
        if not np.isnan(z[f"{case.name}_pl{p}"]).any():
            check_kept(kept, z, case, p)
        assert np.array_equal(kept_var, var)


LOGLIKE_CASES = golden.all_loglike_cases()


@pytest.mark.parametrize("case", LOGLIKE_CASES, ids=[c.name for c in LOGLIKE_CASES])
def test_log_likelihood_rebuilt_from_the_definitions_residuals_is_the_references(case):
    """The reference's logL formula on residuals_definition of the oracle's curves against the log-L the reference itself wrote,
    on all 1506 golden rows: 1e-11 (measured: 2.3e-12 on one row of the eccentricity sweep, at most 4.8e-14 elsewhere), ten times
    inside the bar the device's residuals are held to; NaN rows are exactly the -1e30 rows."""
    res, var = periodogram.residuals_definition(OracleCurves(case), case.theta)
    assert np.array_equal(np.isnan(res).any(axis=1), case.logL == -1e30)
    got = golden.reference_loglike(res, var)
    err = golden.rel_err(got, case.logL)
    print(case.name, "rows", case.theta.shape[0], "invalid", int((case.logL == -1e30).sum()), "largest relative error", float(err.max()))
    assert err.max() <= 1e-11, (case.name, float(err.max()), int(err.argmax()))


def test_the_golden_rows_and_their_invalid_orbits_are_all_there():
    assert sum(c.theta.shape[0] for c in LOGLIKE_CASES) == 1506 and sum(int((c.logL == -1e30).sum()) for c in LOGLIKE_CASES) == 58
