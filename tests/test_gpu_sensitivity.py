"""Prior sensitivity on the device (sensitivity.reweight_arrays / prior_sensitivity with device=0: the ratio table from
rvll_prior_logpdf_batch, reduced by rvll_pointwise_replicates) against the numpy definitions on four synthetic runs.

Bounds: dlogz is an lpd of the pointwise table, held to the pointwise GPU test's 2.5e-10 (tests/test_gpu_pointwise.py: two sums
of non-negative terms good to 1e-10 relative each, and room for the device's exp and log); ln efficiency = 2 lpd - lpd' is three
such logarithms, 7.5e-10; logz to 1e-12 max(1, |logz|) of the definition's, and the bits of merge.replicates_arrays on the
device."""
import math

import numpy as np
import pytest

from evidence_amd import merge, pointwise, priors as P, sensitivity
from test_sensitivity_host import BASE, PARNAMES, _results

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

LPD_BOUND = 2.5e-10
ALTS = [{"a_k1": P.Uniform(0.0, 5.0)}, {"b_period": P.UniformFrequency(1.0, 1000.0)},
        {"c_offset": P.Normal(1.0, 3.0), "a_k1": P.ModJeffreys(1.0, 20.0)},
        {"b_period": P.Jeffreys(2.0, 500.0), "c_offset": P.TruncatedUNormal(0.0, 10.0, -30.0, 30.0)}, {}]


def _close(dev, ref, nrep):
    live = np.isfinite(ref["logz"])
    assert live.any() and np.array_equal(np.isfinite(dev["logz"]), live)
    assert np.all(np.abs(dev["logz"][live] - ref["logz"][live]) <= 1e-12 * np.maximum(1.0, np.abs(ref["logz"][live])))
    err = np.abs(dev["dlogz"][live] - ref["dlogz"][live])
    eff = np.abs(np.log(dev["efficiency"][live]) - np.log(ref["efficiency"][live]))
    print(f"largest dlogz error {err.max():.2e} (bound {LPD_BOUND:.1e}), ln efficiency {eff.max():.2e} (bound {3 * LPD_BOUND:.1e})")
    assert dev["dlogz"].shape == ref["dlogz"].shape == (nrep, len(ALTS))
    assert np.all(err <= LPD_BOUND) and np.all(eff <= 3 * LPD_BOUND)
    assert np.all(np.abs(dev["logz_new"][live] - (dev["logz"][live, None] + dev["dlogz"][live])) == 0.0)
    assert np.array_equal(dev["outside"], ref["outside"])


@pytest.mark.parametrize("mode,bootstrap", [("random", True), ("expected", False)])
def test_the_device_matches_the_definition(gpu_required, mode, bootstrap):
    res = _results(1)
    samples, logl, birth, run_start = pointwise._samples(res)
    ratio = sensitivity.log_ratios(samples, PARNAMES, BASE, ALTS)
    on_device = sensitivity.log_ratios(samples, PARNAMES, BASE, ALTS, device=0)
    assert np.array_equal(np.isneginf(on_device), np.isneginf(ratio))
    f = np.isfinite(ratio)
    base_sets, alt_sets = sensitivity.alternative_sets(PARNAMES, BASE, ALTS)
    sizes = (np.maximum(1.0, np.abs(sensitivity.log_prior_sets(base_sets, samples)))
             + np.maximum(1.0, np.abs(np.where(f, sensitivity.log_prior_sets(alt_sets, samples), 0.0))))
    assert np.all(np.abs(on_device[f] - ratio[f]) <= 1e-10 * sizes[f])              # the difference of two densities at 1e-10 each
    kw = dict(nsamples=37, seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap)
    dev = sensitivity.reweight_arrays(ratio, logl, birth, run_start, device=0, **kw)
    ref = sensitivity.reweight_arrays(ratio, logl, birth, run_start, **kw)
    _close(dev, ref, 37)
    plain = merge.replicates_arrays(logl, birth, run_start, 37, seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap, device=0)
    assert np.array_equal(plain[0], dev["logz"], equal_nan=True) and np.array_equal(plain[1], dev["information"], equal_nan=True)
    assert np.all(np.abs(dev["dlogz"][:, 4]) <= LPD_BOUND) and np.all(np.abs(dev["efficiency"][:, 4] - 1.0) <= 3 * LPD_BOUND)


def test_half_the_width_is_ln_2_and_excluded_rows_are_counted(gpu_required):
    res = _results()
    alts = [{"a_k1": P.Uniform(0.0, 10.0)}, {"a_k1": P.Uniform(0.0, 5.0)}]
    dev = sensitivity.prior_sensitivity(res, PARNAMES, BASE, alts, nsamples=20, seed=7, device=0)
    ref = sensitivity.prior_sensitivity(res, PARNAMES, BASE, alts, nsamples=20, seed=7)
    assert np.all(np.abs(dev["replicates"]["dlogz"][:, 0] - math.log(2.0)) <= LPD_BOUND) and abs(dev["dlogz"][0] - math.log(2.0)) <= LPD_BOUND
    assert dev["outside"][0] == 0 and dev["outside"][1] == ref["outside"][1] > 0
    assert np.all(np.isfinite(dev["replicates"]["dlogz"][:, 1])) and np.isfinite(dev["dlogz"][1])
    assert np.all(np.abs(dev["replicates"]["dlogz"] - ref["replicates"]["dlogz"]) <= LPD_BOUND)
    assert np.all(np.abs(dev["dlogz"] - ref["dlogz"]) <= LPD_BOUND) and np.all(np.abs(dev["dlogz_err"] - ref["dlogz_err"]) <= LPD_BOUND)
    assert np.all(dev["replicates"]["efficiency"][:, 1] < 1.0) and np.all(dev["replicates"]["efficiency"][:, 1] > 0.0)
    assert np.array_equal(np.isneginf(dev["logratio"]), np.isneginf(ref["logratio"]))
