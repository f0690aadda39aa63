"""Residuals of the likelihood's model and their periodograms on the device (GpuRVModel.residuals_batch / gls_bands / gls_batch,
rvll_residuals_batch / rvll_gls_bands; periodogram.residual_gls).

The residuals are held against what the reference's log_likelihood lines give (tests/golden/residuals_51peg.npz) and against the
numpy definition on the device's own curves.  The powers are held against the numpy definition on the device's own residuals in
long double: three float64 evaluations that multiply the phase 2 pi f tau out in different orders differ from it by at most
delta, and the device must lie within 8 delta (a CPU emulation of the kernel's frequency recurrences and sequential sums stayed
within 1.4 delta; the factor leaves room for the device's 1-ulp sincos).  Every step after the powers is a comparison, a pick
or a sum in a fixed order: the order statistics and the peaks must equal the numpy definitions on power_out, and nothing may
depend on the call, the chunking or the other groups.  End to end on a resident 51 Peg ensemble of 8 runs."""
import numpy as np
import pytest

import golden
from evidence_amd import GpuRVModel, _abi, draws, merge, periodogram, predictive, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from evidence_amd.shrinkage import replicate_seeds
from evidence_amd.synthetic import make_workload
from test_gpu_draws import _fragile
from test_gpu_merge import _51peg
from test_gpu_predictive import _ensemble
from test_periodogram_host import check_residuals

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

LEVELS = (0.15865, 0.5, 0.84135)
ORDERS = ("f_tau", "ftau", "tau_f")
N_MAX, F_MAX = 33, 1030
_CACHE = {}


def _extras_model(seed=0):
    """cfg3's table (two instruments) with a drift about the table's first time (a free linear and a fixed quadratic term) and a
    linear activity term: (model arguments, theta sampler)."""
    w = make_workload(3)
    rng = np.random.default_rng(77)
    series = rng.normal(0.0, 1.0, w.table.time.shape[0])
    parnames = sorted(list(w.parnames) + ["drift_lin", "linpar_fwhm"])
    fixed = dict(w.fixedpardict, drift_quad=0.4)

    def sample(n, seed):
        base = w.sample_theta(n, seed)
        r = np.random.default_rng(seed + 1)
        cols = {name: base[:, i] for i, name in enumerate(w.parnames)}
        cols["drift_lin"] = r.uniform(-5.0, 5.0, n)
        cols["linpar_fwhm"] = r.uniform(-2.0, 2.0, n)
        return np.ascontiguousarray(np.stack([cols[name] for name in parnames], axis=1))

    return (fixed, w.table, parnames, {"fwhm": series}), sample


def _open(name):
    if name == "51peg":
        return _51peg()
    if name == "extras":
        args, _ = _extras_model()
        return GpuRVModel(*args)
    w = make_workload(5)
    return GpuRVModel(w.fixedpardict, w.table, w.parnames)


def _theta(name, m, n, seed=11):
    if name == "51peg":
        rng = np.random.default_rng(seed)
        return m.prior_transform_batch(rng.random((n, m.ndim)))
    if name == "extras":
        return _extras_model()[1](n, seed)
    return make_workload(5).sample_theta(n, seed)


def _grid(m):
    span = float(m.table.time.max() - m.table.time.min())
    return 1.0 / span, 1.0 / (8.0 * span)


def _reference(name):
    """Per model, once: theta [n, ndim], the device's residuals, the long-double powers [n, F] and delta (the largest distance
    of the three float64 evaluations from them) for the largest shape; the smaller shapes are its leading rows and frequencies."""
    if name not in _CACHE:
        n, F = (2, 64) if name == "cfg5" else (N_MAX, F_MAX)
        with _open(name) as m:
            theta = _theta(name, m, n)
            res, var = m.residuals_batch(theta)
            time = np.array(m.table.time)
            f0, df = _grid(m)
        assert np.all(np.isfinite(res)) and np.all(var > 0)
        wide = periodogram.gls_definition(time, res, var, f0, df, F, dtype=np.longdouble)
        assert np.all(np.isfinite(wide))
        delta = max(float(np.max(np.abs(periodogram.gls_definition(time, res, var, f0, df, F, phase=o) - wide))) for o in ORDERS)
        _CACHE[name] = dict(theta=theta, wide=wide, delta=delta, f0=f0, df=df, time=time, res=res, var=var)
    return _CACHE[name]


# ---- residuals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden.peg51_cases(), ids=lambda c: c.name)
def test_residuals_match_the_references_log_likelihood_lines(gpu_required, case):
    z = np.load(golden.GOLDEN / "residuals_51peg.npz")
    theta = z[f"{case.name}_theta"]
    with GpuRVModel(case.fixed, case.table, case.parnames) as m:
        res, var = m.residuals_batch(theta)
        one, one_var = m.residuals_batch(theta[1])
        kept, kept_var = m.residuals_batch(theta, keep_planet=1)
    check_residuals(res, var, z, case)
    assert np.array_equal(one[0], res[1]) and np.array_equal(one_var[0], var[1])
    scale = max(np.abs(case.table.vrad).max(), np.abs(z[f"{case.name}_kep"]).max())
    assert np.max(np.abs(kept - (z[f"{case.name}_res"] + z[f"{case.name}_kep"]))) <= 1e-11 * scale
    assert np.array_equal(kept_var, var)


def test_residuals_are_the_definition_on_the_devices_own_curves(gpu_required):
    """Offset, curve, drift and linear terms are added in the definition's order from the same float64 values, so only the drift
    polynomial (a division by 365.25 and powers by repeated multiplication on the device, numpy's ** in the definition) and
    nothing else may round differently: 4 ulp of the largest drift term, and 2 more of the running sum, of magnitude at most
    the sum of the terms' magnitudes."""
    args, sample = _extras_model()
    theta = sample(257, seed=3)
    with GpuRVModel(*args) as m:
        assert m.layout.has_drift and m.layout.tref_from_data and m.layout.has_linpar and len(m.insts) == 2
        for keep in (None, 1, 3):
            res, var = m.residuals_batch(theta, keep_planet=keep)
            want, want_var = periodogram.residuals_definition(m, theta, keep_planet=keep)
            curves = m.kep_rv_batch(theta, m.table.time, exclude_planet=keep)
            tt = (m.table.time - m.table.time[0]) / 365.25
            lin = np.abs(theta[:, m.parnames.index("drift_lin")])[:, None]
            mag = (np.abs(m.table.vrad)[None, :] + 10.0 + np.abs(curves) + lin * np.abs(tt)[None, :] + 0.4 * tt[None, :] ** 2
                   + 2.0 * np.abs(args[3]["fwhm"])[None, :])
            err = np.abs(res - want)
            print("keep_planet", keep, "largest |res - definition| / (magnitude 2^-52):", float(np.max(err / (mag * 2.0 ** -52))))
            assert np.all(err <= 6.0 * 2.0 ** -52 * mag)
            assert np.array_equal(var, want_var)
        with pytest.raises(AssertionError):
            m.residuals_batch(theta, keep_planet=1.0)
        with pytest.raises(ValueError):
            m.residuals_batch(theta[:, :-1])


def test_an_invalid_orbit_gives_a_nan_row_of_residuals(gpu_required):
    cases = {c.name: c for c in golden.edge_cases()}
    bad, good = cases["secos_sesin_invalid"], cases["secos_sesin_ml0"]
    theta = np.concatenate([good.theta[:3], bad.theta[:2], good.theta[3:5]])
    with GpuRVModel(bad.fixed, bad.table, bad.parnames) as m:
        res, var = m.residuals_batch(theta)
        want, want_var = periodogram.residuals_definition(m, theta)
    dead = np.array([False] * 3 + [True] * 2 + [False] * 2)
    assert np.all(np.isnan(res[dead])) and np.all(np.isfinite(res[~dead])) and np.all(np.isfinite(var))
    assert np.array_equal(np.isnan(res), np.isnan(want)) and np.array_equal(var, want_var)


# ---- the powers --------------------------------------------------------------------------------------------------------------
def _check_power(name, n, F):
    ref = _reference(name)
    with _open(name) as m:
        got = m.gls_bands(ref["theta"][None, :n], ref["f0"], ref["df"], F, LEVELS, return_power=True)
        batch = m.gls_batch(ref["theta"][:n], ref["f0"], ref["df"], F)
    power = got["power"][0]
    assert power.shape == (n, F) and np.array_equal(batch, power)
    err = float(np.max(np.abs(power - ref["wide"][:n, :F])))
    print(f"{name} n={n} F={F}: delta {ref['delta']:.3e}, largest |device - long double| {err:.3e}, ratio {err / ref['delta']:.3f}")
    assert np.all(np.isfinite(power)) and err <= 8.0 * ref["delta"]
    q, mean, nv = predictive.bands_definition(got["power"], LEVELS)
    assert np.array_equal(got["q"], q) and np.array_equal(got["mean"], mean) and np.array_equal(got["n_valid"], nv)
    idx, pk = periodogram.peaks_definition(got["power"])
    assert np.array_equal(got["peak_index"], idx) and np.array_equal(got["peak_power"], pk)


@pytest.mark.parametrize("F", [1, 2, 255, 257, 1030])
@pytest.mark.parametrize("n", [1, 5, 33])
@pytest.mark.parametrize("name", ["51peg", "extras"])
def test_powers_lie_within_eight_delta_of_the_long_double_definition(gpu_required, name, n, F):
    _check_power(name, n, F)


def test_powers_of_a_table_of_2000_epochs(gpu_required):
    with _open("cfg5") as m:
        assert m.table.time.shape[0] == 2000                              # epochs pass through LDS in chunks of 256
    _check_power("cfg5", 2, 64)


# ---- independence and the reductions -------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key], equal_nan=True), key


def test_nothing_depends_on_the_call_the_chunking_or_the_other_groups(gpu_required):
    args, sample = _extras_model()
    G, n, F = 5, 7, 600
    theta = sample(G * n, seed=8).reshape(G, n, -1)
    with GpuRVModel(*args) as m:
        f0, df = _grid(m)
        ne = m.table.time.shape[0]
        timing = {}
        first = m.gls_bands(theta, f0, df, F, LEVELS, return_power=True, timing=timing)
        assert timing["gls_ms"] > 0 and timing["residuals_ms"] > 0 and timing["reduce_ms"] > 0
        _same(m.gls_bands(theta, f0, df, F, LEVELS, return_power=True), first)
        group = 8 * n * (F + 2 * ne)
        for chunk in (1, group, 2 * group + 8, 4 * group):                # one group a chunk, one, two, four
            _same(m.gls_bands(theta, f0, df, F, LEVELS, return_power=True, chunk_bytes=chunk), first)
        for g in (0, 3, 4):
            alone = m.gls_bands(theta[g:g + 1], f0, df, F, LEVELS, return_power=True)
            _same(alone, {key: val[g:g + 1] for key, val in first.items()})
        rows = m.gls_batch(theta[2, 1:4], f0, df, F)                      # a row's bits are its own: other rows beside it, another tile
        assert np.array_equal(rows, first["power"][2, 1:4])
        assert np.array_equal(m.gls_batch(theta[1, 5], f0, df, 123), first["power"][1, 5:6, :123])
        kept = m.gls_bands(theta, f0, df, F, LEVELS, keep_planet=2, return_power=True)
        assert not np.array_equal(kept["power"], first["power"])
        assert np.array_equal(m.gls_batch(theta[4], f0, df, F, keep_planet=2), kept["power"][4])


def test_the_reductions_are_the_definitions_with_invalid_orbits_mixed_in(gpu_required):
    cases = {c.name: c for c in golden.edge_cases()}
    bad, good = cases["secos_sesin_invalid"], cases["secos_sesin_ml0"]
    rng = np.random.default_rng(2)
    mixed = np.concatenate([good.theta, bad.theta])[rng.permutation(30)]
    theta = np.stack([mixed, np.resize(bad.theta, (30, bad.theta.shape[1])), np.resize(good.theta, (30, good.theta.shape[1]))])
    with GpuRVModel(bad.fixed, bad.table, bad.parnames) as m:
        f0, df = _grid(m)
        for F, levels in ((1, [0.5]), (45, LEVELS), (700, np.linspace(0.01, 0.99, 16))):
            got = m.gls_bands(theta, f0, df, F, levels, return_power=True)
            q, mean, nv = predictive.bands_definition(got["power"], levels)
            assert np.array_equal(got["q"], q, equal_nan=True) and np.array_equal(got["mean"], mean, equal_nan=True)
            assert got["n_valid"].dtype == np.int32 and np.array_equal(got["n_valid"], nv)
            idx, pk = periodogram.peaks_definition(got["power"])
            assert got["peak_index"].dtype == np.int32 and np.array_equal(got["peak_index"], idx)
            assert np.array_equal(got["peak_power"], pk, equal_nan=True)
            assert np.all(nv[0] == 24) and np.all(nv[1] == 0) and np.all(nv[2] == 30)
            assert np.all(np.isnan(got["q"][1])) and np.all(np.isnan(got["mean"][1])) and np.all(got["peak_index"][1] == -1)
            assert np.all(np.isfinite(got["q"][0])) and np.sum(got["peak_index"][0] == -1) == 6 and np.all(got["peak_index"][2] >= 0)
            without = m.gls_bands(theta, f0, df, F, levels)
            assert "power" not in without
            for key in without:
                assert np.array_equal(without[key], got[key], equal_nan=True), key


def test_refusals(gpu_required):
    w = make_workload(2)
    theta = w.sample_theta(8, seed=1)
    levels = np.array([0.5])
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        f0, df = _grid(m)
        q, mean, nv = np.zeros(64), np.zeros(64), np.zeros(64, np.int32)
        pidx, ppow, power = np.zeros(64, np.int32), np.zeros(64), np.zeros(256)

        def raw(G=2, n=4, f0=f0, df=df, F=3, lv=levels, nq=1, chunk=0, null=()):
            lv = np.ascontiguousarray(lv, dtype=np.float64)
            return m._lib.rvll_gls_bands(m._h, None if "theta" in null else _abi.as_dp(theta), G, n, 1, f0, df, F,
                                         None if "levels" in null else _abi.as_dp(lv), nq,
                                         None if "q" in null else _abi.as_dp(q), None if "mean" in null else _abi.as_dp(mean),
                                         None if "n_valid" in null else _abi.as_ip(nv),
                                         None if "peak_index" in null else _abi.as_ip(pidx),
                                         None if "peak_power" in null else _abi.as_dp(ppow),
                                         None if "power" in null else _abi.as_dp(power), chunk, None)

        assert raw() == _abi.OK and raw(G=0) == _abi.OK and raw(null=("power",)) == _abi.OK
        for bad in (dict(f0=0.0), dict(f0=-0.1), dict(f0=np.nan), dict(df=0.0), dict(df=-0.1), dict(df=np.inf), dict(F=0), dict(F=-1),
                    dict(n=0), dict(n=4097), dict(n=-1), dict(nq=0), dict(nq=17), dict(lv=[0.0]), dict(lv=[1.0]), dict(lv=[np.nan]),
                    dict(lv=[0.5, 1.5], nq=2), dict(G=-1), dict(chunk=-1), dict(null=("theta",)), dict(null=("levels",)),
                    dict(null=("q",)), dict(null=("mean",)), dict(null=("n_valid",)), dict(null=("peak_index",)),
                    dict(null=("peak_power",))):
            assert raw(**bad) == _abi.E_INVALID, bad
        res, var = np.zeros((8, 200)), np.zeros((8, 200))
        lib = m._lib.rvll_residuals_batch
        assert lib(m._h, _abi.as_dp(theta), 8, 1, _abi.as_dp(res), _abi.as_dp(var)) == _abi.OK
        assert lib(m._h, _abi.as_dp(theta), 0, 1, None, None) == _abi.OK
        assert lib(m._h, _abi.as_dp(theta), -1, 1, _abi.as_dp(res), _abi.as_dp(var)) == _abi.E_INVALID
        assert lib(m._h, None, 8, 1, _abi.as_dp(res), _abi.as_dp(var)) == _abi.E_INVALID
        assert lib(m._h, _abi.as_dp(theta), 8, 1, None, _abi.as_dp(var)) == _abi.E_INVALID
        assert lib(m._h, _abi.as_dp(theta), 8, 1, _abi.as_dp(res), None) == _abi.E_INVALID
        for bad in (dict(f0=0.0), dict(df=-1.0), dict(nfreq=0)):
            kw = dict(f0=f0, df=df, nfreq=3)
            kw.update(bad)
            with pytest.raises(ValueError):
                m.gls_bands(theta.reshape(2, 4, -1), levels=[0.5], **kw)
        with pytest.raises(ValueError):
            m.gls_bands(theta.reshape(2, 4, -1), f0, df, 3, [1.0])
        with pytest.raises(ValueError):
            m.gls_bands(theta, f0, df, 3, [0.5])                          # not [G, n, ndim]
    few = w.table.time[:3]
    from evidence_amd.data import EpochTable
    small = EpochTable.from_arrays(list(w.table.insts), few, w.table.vrad[:3], w.table.svrad[:3], np.zeros(3, np.int32))
    with GpuRVModel(w.fixedpardict, small, w.parnames) as m:              # fewer than 4 epochs
        assert m._lib.rvll_gls_bands(m._h, _abi.as_dp(theta), 2, 4, 1, 0.01, 0.01, 3, _abi.as_dp(levels), 1, _abi.as_dp(q),
                                     _abi.as_dp(mean), _abi.as_ip(nv), _abi.as_ip(pidx), _abi.as_dp(ppow), None, 0,
                                     None) == _abi.E_INVALID
        with pytest.raises(ValueError, match="epochs"):
            m.gls_bands(theta.reshape(2, 4, -1), 0.01, 0.01, 3, [0.5])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _peg_k0():
    from pathlib import Path
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=0)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def _ensemble_k0():
    """8 resident runs of the 51 Peg model without a planet, made once for the module."""
    if "k0" not in _CACHE:
        with _peg_k0() as m:
            assert m.nplanets == 0
            _CACHE["k0"] = run_nested_ensemble(None, None, m.ndim, list(range(1, 9)), live=m, nlive=400, dlogz=0.5,
                                               wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
    return _CACHE["k0"]


def test_the_residual_periodogram_of_51_peg_with_and_without_its_planet(gpu_required):
    one, _ = _ensemble()
    zero = _ensemble_k0()
    with _peg_k0() as m0:
        # down to the prior's shortest period, 1.5 d (the default, twice the median spacing of these clustered nights, is 0.027 d:
        # 292502 frequencies)
        f0, df, nfreq = periodogram.frequency_grid(m0.table.time, pmin=1.5)
        kw = dict(f0=f0, df=df, nfreq=nfreq, ndraws=128, nsamples=40, seed=5, device=0)
        none = periodogram.residual_gls(zero, m0, **kw)
    with _51peg() as m1:
        left = periodogram.residual_gls(one, m1, **kw)
        back = periodogram.residual_gls(one, m1, keep_planet=1, **kw)
    freq = none["freq"]
    assert freq.shape == (nfreq,) and freq[0] == f0 and np.array_equal(left["freq"], freq) and np.array_equal(none["period"], 1.0 / freq)
    near = int(np.argmin(np.abs(freq - 1.0 / 4.2308)))
    top0, top_back = int(np.argmax(none["band"][1])), int(np.argmax(back["band"][1]))
    print("grid", nfreq, "frequencies; 1 / 4.2308 d at index", near, "; median band's top without a planet at", top0,
          "with the planet kept at", top_back, "; median power there:", float(none["band"][1][top0]), "residual model:",
          float(left["band"][1][near]), "peak_fraction:", float(none["peak_fraction"][top0]))
    assert abs(top0 - near) <= 1 and abs(int(np.argmax(none["peak_fraction"])) - near) <= 1
    assert left["band"][1][top0] < none["band"][0][top0]                  # the planet's model takes the peak out ...
    assert abs(top_back - near) <= 1 and abs(int(np.argmax(back["peak_fraction"])) - near) <= 1       # ... and keep_planet leaves it in
    for out in (none, left, back):
        assert out["band"].shape == (3, nfreq) and out["replicates"] == 40 and np.all(out["n_valid_min"] == 128)
        assert np.all(out["band_min"] <= out["band"]) and np.all(out["band"] <= out["band_max"]) and np.all(out["band_err"] >= 0)
        assert np.all(out["band"][0] <= out["band"][1]) and np.all(out["band"][1] <= out["band"][2])
        assert abs(out["peak_fraction"].sum() - 1.0) <= 1e-12 and np.all(out["peak_fraction_err"] >= 0)


def test_the_device_and_the_numpy_route_agree_on_every_replicate(gpu_required):
    """band of device=0 against device=None: the powers differ by at most 8 delta, so the picked order statistic is the same
    draw's — and within 8 delta — wherever the definition's pick is further than that from its neighbours in the sorted column;
    the entries where it is not are left out, and the definition alone must keep them below 1 in 1000."""
    results, _ = _ensemble()
    S, n, F = 12, 64, 300
    kw = dict(ndraws=n, nsamples=S, seed=3, return_replicates=True)
    _, logl, birth, run_start = merge._stack(results)
    with _51peg() as m:
        f0, df = _grid(m)
        dev = periodogram.residual_gls(results, m, f0, df, F, device=0, **kw)
        ref = periodogram.residual_gls(results, m, f0, df, F, device=None, **kw)
        theta = draws.samples(results, n, S, 3, "random", True, None)
        res, var = m.residuals_batch(theta.reshape(S * n, -1))
        time = np.array(m.table.time)
    logwt = merge.replicates_arrays(logl, birth, run_start, S, seed=3, return_logwt=True)[2]
    c_def = np.cumsum(draws.fixed_point(logwt), axis=1, dtype=np.int64)
    seeds = replicate_seeds(3, S)
    frag = np.array([_fragile(c_def[s], seeds[s], n) for s in range(S)])
    sound = ~frag.any(axis=1)
    assert frag.sum() * 1000 <= frag.size and np.all(dev["alive"]) and np.all(ref["alive"])
    wide = periodogram.gls_definition(time, res, var, f0, df, F, dtype=np.longdouble)
    evals = [periodogram.gls_definition(time, res, var, f0, df, F, phase=o) for o in ORDERS]
    delta = max(float(np.max(np.abs(e - wide))) for e in evals)
    bound = 8.0 * delta
    power = evals[0].reshape(S, n, F)
    srt = np.sort(power, axis=1)
    gaps = np.diff(srt, axis=1)                                           # [S, n - 1, F]
    unsure = np.zeros((S, len(LEVELS), F), dtype=bool)
    for k, lv in enumerate(LEVELS):
        idx = int(np.ceil(lv * float(n))) - 1
        unsure[:, k, :] = (gaps[:, idx - 1, :] <= bound) | (gaps[:, idx, :] <= bound)
    print("delta", delta, "entries left out:", int(unsure.sum()), "of", unsure.size, "; sound replicates:", int(sound.sum()), "of", S)
    assert unsure.sum() * 1000 <= unsure.size
    assert np.array_equal(ref["q"], predictive.bands_definition(power, LEVELS)[0])
    keep = ~unsure & sound[:, None, None]
    assert np.all(np.abs(dev["q"] - ref["q"])[keep] <= bound)
    assert np.all(np.abs(dev["mean_replicates"] - ref["mean_replicates"])[sound] <= bound)
    if sound.all() and not unsure.any():
        assert np.max(np.abs(dev["band"] - ref["band"])) <= bound
