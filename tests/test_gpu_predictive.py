"""Curve bands and phase folds on the device (GpuRVModel.kep_rv_bands, rvll_kep_rv_bands; predictive.curve_bands / phase_fold).

The band kernel sorts the very values that kep_rv_batch returns (the same curve kernel writes them into a device buffer), and
every step after that is a comparison, a pick, or a sum in a fixed order: q, mean and n_valid must equal the numpy definition
applied to kep_rv_batch's output as float64 values, NaN positions included, for group sizes on both sides of the powers of two
and of the time tile, in any chunking.  End to end on a resident 51 Peg ensemble of 8 runs, where the draws of a replicate that
is not fragile (tests/test_gpu_draws.py) are the definition's and so its band is too."""
import ctypes as C

import numpy as np
import pytest

import golden
from evidence_amd import GpuRVModel, _abi, draws, merge, posterior, predictive, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from evidence_amd.shrinkage import replicate_seeds
from evidence_amd.synthetic import make_workload
from test_gpu_draws import _fragile
from test_gpu_merge import _51peg
from test_predictive_host import check_fold

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

LEVELS = (0.15865, 0.5, 0.84135)
_ENSEMBLE = {}


def _same(got, want):
    for a, b, name in zip(got, want, ("q", "mean", "n_valid")):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name


def test_bands_are_the_definition_on_kep_rv_batchs_values_in_any_chunking(gpu_required):
    w = make_workload(3)
    G = 5
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        for n in (1, 2, 63, 256, 257, 1000):
            theta = w.sample_theta(G * n, seed=100 + n).reshape(G, n, -1)
            for T in (1, 17, 130):
                times = np.linspace(50000.0, 50900.0, T) if T > 1 else np.array([50123.25])
                curves = m.kep_rv_batch(theta.reshape(G * n, -1), times, exclude_planet=2).reshape(G, n, T)
                want = predictive.bands_definition(curves, LEVELS)
                timing = {}
                got = m.kep_rv_bands(theta, times, LEVELS, exclude_planet=2, timing=timing)
                _same(got, want)
                assert got[2].dtype == np.int32 and np.all(got[2] == n) and timing["sort_ms"] > 0
                _same(m.kep_rv_bands(theta, times, LEVELS, exclude_planet=2, chunk_bytes=8 * n * T), want)     # a group a chunk
                _same(m.kep_rv_bands(theta, times, LEVELS, exclude_planet=2, chunk_bytes=8 * n * T * 2 + 8), want)
        theta = w.sample_theta(3 * 40, seed=5).reshape(3, 40, -1)
        times = np.linspace(50000.0, 50100.0, 33)
        for planet in (1, 2, 3):
            curves = m.modelk_batch(theta.reshape(120, -1), times, planet).reshape(3, 40, 33)
            _same(m.kep_rv_bands(theta, times, [0.5], planet=planet), predictive.bands_definition(curves, [0.5]))
        sixteen = np.linspace(0.01, 0.99, 16)
        curves = m.kep_rv_batch(theta.reshape(120, -1), times).reshape(3, 40, 33)
        _same(m.kep_rv_bands(theta, times, sixteen), predictive.bands_definition(curves, sixteen))


def test_invalid_orbits_are_counted_out_and_a_group_of_them_is_nan(gpu_required):
    cases = {c.name: c for c in golden.edge_cases()}
    bad, good = cases["secos_sesin_invalid"], cases["secos_sesin_ml0"]
    assert bad.parnames == good.parnames and bad.fixed == good.fixed
    rng = np.random.default_rng(2)
    mixed = np.concatenate([good.theta, bad.theta])[rng.permutation(30)]
    theta = np.stack([mixed, np.resize(bad.theta, (30, bad.theta.shape[1])), np.resize(good.theta, (30, good.theta.shape[1]))])
    times = np.linspace(49990.0, 50410.0, 19)
    with GpuRVModel(bad.fixed, bad.table, bad.parnames) as m:
        curves = m.kep_rv_batch(theta.reshape(90, -1), times).reshape(3, 30, 19)
        got = m.kep_rv_bands(theta, times, LEVELS)
    _same(got, predictive.bands_definition(curves, LEVELS))
    q, mean, nv = got
    assert np.all(nv[0] == 24) and np.all(nv[1] == 0) and np.all(nv[2] == 30)
    assert np.all(np.isnan(q[1])) and np.all(np.isnan(mean[1])) and np.all(np.isfinite(q[0])) and np.all(np.isfinite(mean[0]))


def test_the_eccentricity_sweep_as_one_group(gpu_required):
    case = golden.high_ecc_case()                                         # wandering solves from e = 0.97 on
    t = np.linspace(case.table.time.min() - 30, case.table.time.max() + 30, 997)
    theta = case.theta[None]
    assert theta.shape[1] == 240
    with GpuRVModel(case.fixed, case.table, case.parnames) as m:
        curves = m.kep_rv_batch(case.theta, t)[None]
        _same(m.kep_rv_bands(theta, t, LEVELS), predictive.bands_definition(curves, LEVELS))
        _same(m.kep_rv_bands(theta, t, LEVELS, planet=1), predictive.bands_definition(m.modelk_batch(case.theta, t, 1)[None], LEVELS))


def test_refusals(gpu_required):
    w = make_workload(2)
    theta = w.sample_theta(8, seed=1)
    times, levels = np.array([50000.0, 50001.0]), np.array([0.5])
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        q, mean, nv = np.zeros(64), np.zeros(64), np.zeros(64, np.int32)

        def raw(G=2, n=4, T=2, lv=levels, nq=1, chunk=0, null=()):
            lv = np.ascontiguousarray(lv, dtype=np.float64)
            return m._lib.rvll_kep_rv_bands(m._h, None if "theta" in null else _abi.as_dp(theta), G, n,
                                            None if "times" in null else _abi.as_dp(times), T, 1,
                                            None if "levels" in null else _abi.as_dp(lv), nq,
                                            None if "q" in null else _abi.as_dp(q), None if "mean" in null else _abi.as_dp(mean),
                                            None if "n_valid" in null else _abi.as_ip(nv), chunk, None)

        assert raw() == _abi.OK and raw(G=0) == _abi.OK and raw(T=0) == _abi.OK
        for bad in (dict(n=0), dict(n=4097), dict(n=-1), dict(nq=0), dict(nq=17), dict(lv=[0.0]), dict(lv=[1.0]), dict(lv=[np.nan]),
                    dict(lv=[0.5, 1.5], nq=2), dict(G=-1), dict(T=-1), dict(chunk=-1), dict(null=("theta",)), dict(null=("times",)),
                    dict(null=("levels",)), dict(null=("q",)), dict(null=("mean",)), dict(null=("n_valid",))):
            assert raw(**bad) == _abi.E_INVALID, bad
        with pytest.raises(ValueError):
            m.kep_rv_bands(theta.reshape(2, 4, -1), times, [1.0])
        with pytest.raises(ValueError):
            m.kep_rv_bands(theta, times, [0.5])                           # not [G, n, ndim]
        with pytest.raises(KeyError):
            m.kep_rv_bands(theta.reshape(2, 4, -1), times, [0.5], planet=2)


def _ensemble():
    """8 resident 51 Peg runs, made once for the module: (results, parnames)."""
    if not _ENSEMBLE:
        with _51peg() as m:
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, 9)), live=m, nlive=400, dlogz=0.5,
                                      wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
            _ENSEMBLE.update(results=got, names=list(m.parnames))
    return _ENSEMBLE["results"], _ENSEMBLE["names"]


def test_curve_bands_on_the_device_are_the_definitions_on_every_replicate_that_is_not_fragile(gpu_required):
    results, _ = _ensemble()
    S, n = 12, 64
    kw = dict(planet=1, ndraws=n, nsamples=S, seed=3, return_replicates=True)
    _, logl, birth, run_start = merge._stack(results)
    times = np.linspace(50000.0, 50009.0, 41)
    with _51peg() as m:
        dev = predictive.curve_bands(results, m, times, device=0, **kw)
        ref = predictive.curve_bands(results, m, times, device=None, **kw)
    logwt = merge.replicates_arrays(logl, birth, run_start, S, seed=3, return_logwt=True)[2]
    c_def = np.cumsum(draws.fixed_point(logwt), axis=1, dtype=np.int64)
    seeds = replicate_seeds(3, S)
    frag = np.array([_fragile(c_def[s], seeds[s], n) for s in range(S)])
    sound = ~frag.any(axis=1)
    print("fragile draws:", int(frag.sum()), "of", frag.size, "; replicates without one:", int(sound.sum()), "of", S)
    assert frag.sum() * 1000 <= frag.size and np.all(dev["alive"]) and np.all(ref["alive"])
    assert np.array_equal(dev["q"][sound], ref["q"][sound]) and np.array_equal(dev["mean_replicates"][sound],
                                                                                ref["mean_replicates"][sound])
    if sound.all():
        for key in ("band", "band_err", "band_min", "band_max", "mean", "mean_err", "n_valid_min"):
            assert np.array_equal(dev[key], ref[key]), key
    assert dev["band"].shape == (3, 41) and np.all(dev["band_min"] <= dev["band"]) and np.all(dev["band"] <= dev["band_max"])
    assert np.all(dev["band"][0] <= dev["band"][1]) and np.all(dev["band"][1] <= dev["band"][2]) and np.all(dev["band_err"] >= 0)
    assert np.all(dev["n_valid_min"] == n)


def test_the_phase_fold_of_51_peg_b(gpu_required):
    results, names = _ensemble()
    with _51peg() as m:
        fold = predictive.phase_fold(results, m, names, 1, nphase=200, ndraws=256, nsamples=100, seed=7, device=0)
    tab = posterior.table(results, names, nsamples=100, seed=7, device=0)
    k = names.index("planet1_k1")
    k1, k1_err = float(tab["mean"][k]), float(tab["mean_err"][k])
    median = fold["band"][1]
    amplitude = 0.5 * (median.max() - median.min())
    print("k1", k1, "+/-", k1_err, "amplitude of the median curve", amplitude, "largest band_err", float(fold["band_err"].max()))
    assert abs(amplitude - k1) <= 5.0 * k1_err
    assert fold["phase"].shape == (200,) and fold["band"].shape == (3, 200) and fold["replicates"] == 100
    data = fold["data"]
    assert data["phase"].shape == data["rv"].shape == data["rv_err"].shape and abs(data["period"] - 4.2308) < 1e-3
    assert np.array_equal(fold["theta"], tab["mean"])


@pytest.mark.parametrize("case", golden.peg51_cases(), ids=lambda c: c.name)
def test_phase_fold_data_matches_the_references_loop_on_the_devices_curves(gpu_required, case):
    z = np.load(golden.GOLDEN / "phasefold_51peg.npz")
    with GpuRVModel(case.fixed, case.table, case.parnames) as m:
        got = predictive.phase_fold_data(m, z[f"{case.name}_theta"], 1)
    check_fold(got, z, case.name)
