"""GPU: the reduced-precision modes (BASELINE.json configs[4]: fp32 vs fp64 tolerance sweep).
They are NOT parity modes; these tests pin how far they are from the fp64 path and that the fp64
path is untouched by their existence."""
import numpy as np
import pytest

import golden
from evidence_amd import GpuRVModel
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]


def _run(w, theta, precision):
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, precision=precision) as m:
        return m.log_likelihood_batch(theta)


# (max, median) of the relative log-L error against the fp64 path, per config and mode: at most 5x what was measured on
# the MI355X for these very samples (profiles/DESIGN_history_r1_r3.md §4 table; max 1.2e-7 / 1.4e-7 / 9.2e-8 for cfg2 / 3 / 5, medians 2.0e-10 ..
# 3.5e-8), so a regression by an order of magnitude fails.  With sincos_f32's pi/2 split exact in float the maxima of cfg2 and
# cfg5 fell (1.20e-7 / 1.20e-7 -> 1.03e-7 / 9.93e-8 and 9.63e-8 / 9.99e-8 -> 6.57e-8 / 6.38e-8) and their bounds with them, by the
# same rule; cfg3's single worst sample moved the other way (1.49e-7 / 1.75e-7 -> 1.72e-7 / 1.85e-7): its bounds stay
BOUNDS = {
    (2, "mixed"): (5.2e-7, 1.0e-9), (2, "fp32"): (5.0e-7, 1.8e-7),
    (3, "mixed"): (7e-7, 1.6e-8), (3, "fp32"): (7.5e-7, 1.7e-7),
    (5, "mixed"): (3.3e-7, 1.2e-8), (5, "fp32"): (3.2e-7, 5.5e-8),
}


@pytest.mark.parametrize("cfg,n", [(2, 4096), (3, 8192), (5, 1024)])
def test_tolerance_sweep(gpu_required, cfg, n):
    w = make_workload(cfg)
    theta = w.sample_theta(n, seed=321 + cfg)
    ref = _run(w, theta, "fp64")
    for precision in ("mixed", "fp32"):
        bound_max, bound_med = BOUNDS[(cfg, precision)]
        got = _run(w, theta, precision)
        err = golden.rel_err(got, ref)
        print(f"cfg{cfg} {precision}: max {err.max():.2e} median {np.median(err):.2e} p99 {np.percentile(err, 99):.2e} "
              f"max abs {np.max(np.abs(got - ref)):.3e}")
        assert err.max() <= bound_max and np.median(err) <= bound_med, (cfg, precision, float(err.max()), float(np.median(err)))


def test_reduced_precision_keeps_sentinels_and_phase_range(gpu_required):
    # the invalid-orbit sentinel and the |M| ~ 1e4 rad phase (51Peg: t - epoch ~ 1000 d, P ~ 4 d) survive
    for case in golden.edge_cases():
        if case.name == "secos_sesin_invalid":
            with GpuRVModel(case.fixed, case.table, case.parnames, precision="mixed") as m:
                assert np.all(m.log_likelihood_batch(case.theta) == -1e30)
    case = golden.peg51_cases()[0]
    with GpuRVModel(case.fixed, case.table, case.parnames, precision="mixed") as m:
        got = m.log_likelihood_batch(case.theta)
    assert golden.rel_err(got, case.logL).max() <= 2e-5


def test_fp64_is_default_and_unchanged(gpu_required):
    case = golden.config_case(3)
    with GpuRVModel(case.fixed, case.table, case.parnames) as m:
        assert m.precision == "fp64"
        assert golden.rel_err(m.log_likelihood_batch(case.theta), case.logL).max() <= 1e-10
    with pytest.raises(ValueError):
        GpuRVModel(case.fixed, case.table, case.parnames, precision="bf16")


@pytest.mark.parametrize("precision", ["mixed", "fp32"])
def test_reduced_precision_does_not_fall_apart_at_the_eccentricity_clamp(gpu_required, precision):
    """The eccentricity sweep of the golden set (one planet at 0.90 .. 0.9925): where the solver's iteration wanders far
    outside what a float can follow, the reduced-precision modes hand that solve to the double path instead of returning
    whatever a float iteration ends on; against the reference's own numbers the sweep stays within the modes' tolerance
    class (not a parity mode: 1e-10 is for precision="fp64")."""
    import golden
    case = golden.high_ecc_case()
    with GpuRVModel(case.fixed, case.table, case.parnames, precision=precision) as m:
        got = m.log_likelihood_batch(case.theta)
    err = golden.rel_err(got, case.logL)
    assert np.isfinite(got).all()
    z = np.load(golden.GOLDEN / "loglike_high_ecc.npz")
    ecc = z["ecc_of_row"]
    assert err[ecc <= 0.95].max() <= 1e-4, float(err[ecc <= 0.95].max())
    assert err.max() <= 0.1, float(err.max())       # at the clamp 1 / f' ~ 100 multiplies a float's 1e-7 on E into 1e-2 on log-L
    assert np.median(err) <= 1e-5, float(np.median(err))


@pytest.mark.parametrize("precision", ["mixed", "fp32"])
def test_item_pairs_and_single_items_agree_to_float_rounding(gpu_required, precision):
    """Round 4: with the reference's itmax (10000) the reduced-precision modes evaluate two items a lane with a wave-wide stop rule
    (rvll_tile.h, eval_item_pair); an itmax of 16 or less keeps the single-item path (its per-item stop counts against itmax).
    Same points, both paths: the same values to a few float ulps of the model wherever no solve comes near sixteen steps, and
    the same flags."""
    case = golden.config_case(3)
    theta = np.tile(case.theta, (30, 1))
    out = {}
    for itmax in (16, 10000):
        with GpuRVModel(case.fixed, case.table, case.parnames, precision=precision, itmax=itmax) as m:
            out[itmax] = m.log_likelihood_batch(theta, return_flags=True)
    assert np.array_equal(out[16][1], out[10000][1])
    assert (out[16][1] == 0).all()
    assert golden.rel_err(out[16][0], out[10000][0]).max() <= 3e-7
    assert golden.rel_err(out[10000][0], np.tile(case.logL, 30)).max() <= 1e-6
