"""CPU: the numpy definitions of evidence_amd/predictive.py.  The order statistics of groups of curves against a per-column Python
loop, NaNs included, and at the quantile boundaries; refusals; the prototype of the device entry; phase_fold_data on the oracle's
curves against what the reference's own phase-fold loop gives for the two shipped 51 Peg configurations
(tests/golden/phasefold_51peg.npz, made by gen_phasefold_golden.py)."""
import math

import numpy as np
import pytest

import golden
from evidence_amd import _abi, predictive

LEVELS = (0.15865, 0.5, 0.84135)


def _loop(values, levels):
    G, n, T = values.shape
    q, mean, nv = np.full((G, len(levels), T), np.nan), np.full((G, T), np.nan), np.zeros((G, T), np.int32)
    for g in range(G):
        for j in range(T):
            v = sorted(float(x) for x in values[g, :, j] if not math.isnan(x))
            nv[g, j] = len(v)
            if not v:
                continue
            for k, lv in enumerate(levels):
                q[g, k, j] = v[max(0, math.ceil(lv * float(len(v))) - 1)]
            total = v[0]
            for x in v[1:]:
                total += x
            mean[g, j] = total / len(v)
    return q, mean, nv


@pytest.mark.parametrize("n", [1, 2, 7, 63, 257])
def test_the_definition_matches_a_loop_over_columns_with_nans(n):
    rng = np.random.default_rng(n)
    values = rng.normal(0.0, 30.0, (4, n, 9))
    values[rng.random(values.shape) < 0.2] = np.nan
    values[1, :, 3] = np.nan                                              # a column without a valid curve
    values[2] = np.nan                                                    # a group without one
    values[3, :, 0] = np.round(values[3, :, 0])                           # ties
    got = predictive.bands_definition(values, LEVELS)
    want = _loop(values, LEVELS)
    assert got[2].dtype == np.int32
    for a, b in zip(got, want):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.all(np.isnan(got[0][2])) and np.all(np.isnan(got[1][2])) and np.all(got[2][2] == 0)


def test_a_level_on_a_quantile_boundary():
    values = np.array([3.0, 1.0, 4.0, 2.0]).reshape(1, 4, 1)
    q, mean, nv = predictive.bands_definition(values, [0.5, 0.5000001, 0.25, 0.2500001, 0.999, 1e-9])
    assert list(q[0, :, 0]) == [2.0, 3.0, 1.0, 2.0, 4.0, 1.0] and mean[0, 0] == 2.5 and nv[0, 0] == 4
    values = np.array([3.0, np.nan, 4.0, 2.0, 1.0, np.nan]).reshape(1, 6, 1)      # the boundaries are those of the valid rows
    q, mean, nv = predictive.bands_definition(values, [0.5, 0.5000001])
    assert list(q[0, :, 0]) == [2.0, 3.0] and nv[0, 0] == 4


def test_refusals_and_the_prototypes():
    ok = np.zeros((1, 2, 3))
    for bad in ([], [0.0], [1.0], [0.5, np.nan], [-0.1], list(np.linspace(0.1, 0.9, 17))):
        with pytest.raises(ValueError, match="levels"):
            predictive.bands_definition(ok, bad)
    predictive.bands_definition(ok, list(np.linspace(0.1, 0.9, 16)))
    with pytest.raises(ValueError, match="rows"):
        predictive.bands_definition(np.zeros((1, 4097, 1)), [0.5])
    with pytest.raises(ValueError, match="rows"):
        predictive.bands_definition(np.zeros((1, 0, 1)), [0.5])
    predictive.bands_definition(np.zeros((1, 4096, 1)), [0.5])
    with pytest.raises(ValueError, match="groups"):
        predictive.bands_definition(np.zeros((4, 3)), [0.5])
    assert "rvll_kep_rv_bands" in _abi.PROTOTYPES and "rvll_draw_replicates" in _abi.PROTOTYPES
    lib = _abi.load()
    assert hasattr(lib, "rvll_kep_rv_bands") and hasattr(lib, "rvll_draw_replicates")


class OracleCurves:
    """What phase_fold_data needs of a model, with the curves of the CPU oracle."""

    def __init__(self, case):
        from oracle.oracle import OracleModel
        self.layout, self.table, self.linpar_dict = case.layout, case.table, case.linpar
        self._oracle = OracleModel(case.layout, case.table, case.linpar_series)

    def kep_rv_batch(self, X, time, exclude_planet=None):
        mask = (1 << self.layout.nplanets) - 1
        if exclude_planet is not None:
            mask &= ~(1 << (exclude_planet - 1))
        return self._oracle.kep_rv(X, time, mask)

    def modelk_batch(self, X, time, planet):
        return self._oracle.kep_rv(X, time, 1 << (planet - 1))


def check_fold(got, z, name):
    """phase_fold_data against the fixture: phases to 1e-12 d, everything that holds a curve to 1e-11 of the curve's amplitude
    (the bound tests/test_gpu_curves.py holds the curves to), the rest exactly."""
    amp = np.abs(z[f"{name}_model"]).max()
    assert got["t_ref"] == float(z[f"{name}_t_ref"]) and got["period"] == float(z[f"{name}_period"])
    assert np.max(np.abs(got["phase"] - z[f"{name}_phase"])) <= 1e-12
    assert np.max(np.abs(got["rv"] - z[f"{name}_rv"])) <= 1e-11 * amp
    assert np.max(np.abs(got["model"] - z[f"{name}_model"])) <= 1e-11 * amp
    assert np.array_equal(got["rv_err"], z[f"{name}_rv_err"]) and np.array_equal(got["inst"], z[f"{name}_inst"])


@pytest.mark.parametrize("case", golden.peg51_cases(), ids=lambda c: c.name)
def test_phase_fold_data_matches_the_references_loop_on_the_oracles_curves(case):
    z = np.load(golden.GOLDEN / "phasefold_51peg.npz")
    got = predictive.phase_fold_data(OracleCurves(case), z[f"{case.name}_theta"], 1)
    check_fold(got, z, case.name)
    assert (case.name == "51peg_drift") == case.layout.has_drift
    assert np.all(got["phase"] >= -0.5 * got["period"]) and np.all(got["phase"] < 0.5 * got["period"])
    with pytest.raises(KeyError):
        predictive.phase_fold_data(OracleCurves(case), z[f"{case.name}_theta"], 2)
    with pytest.raises(ValueError, match="parameters"):
        predictive.phase_fold_data(OracleCurves(case), z[f"{case.name}_theta"][:-1], 1)
