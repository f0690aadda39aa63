"""CPU: the FIP periodogram of merged runs (evidence_amd/fip.py: merged_tip_arrays, merged_fip).  The numpy definition against
the reference's own accumulation loop (oracle.fip_oracle.accumulate) fed with the replicate's weights as one run; the union of a
row's spans; a tiling grid on which the inclusion probabilities of a one-planet model sum to one; the combination of the models;
the argument checks; and the built library's export of rvll_fip_replicates."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import _abi, fip, merge
from evidence_amd.nested import NestedResult
from oracle import fip_oracle
from test_merge_host import _arrays, _ragged


def _grid(nfreq=300, tobs=40.0):
    return fip.frequency_grid(1.5, 200.0, tobs, nfreq=nfreq)


def _periods(n, nplanets, seed):
    """Periods of n rows: a peak at 4.23 d, a second column mostly next to the first (overlapping, adjacent and separate
    spans), a third spread over the whole grid and beyond its ends."""
    rng = np.random.default_rng(seed)
    p1 = 4.23 * (1.0 + 0.05 * rng.normal(size=n))
    p2 = p1 * (1.0 + 0.02 * rng.normal(size=n))
    p3 = np.exp(rng.uniform(np.log(1.2), np.log(400.0), n))
    return np.abs(np.stack([p1, p2, p3], axis=1)[:, :nplanets]) + 0.5


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
@pytest.mark.parametrize("nplanets", [1, 2, 3])
def test_definition_matches_the_reference_loop_on_the_replicates_weights(nplanets, mode, bootstrap):
    logl, birth, run_start = _arrays(_ragged(3))
    n = logl.size
    periods = _periods(n, nplanets, 10 + nplanets)
    _, nua, nub = _grid()
    kw = dict(nsamples=5, seed=2 ** 64 - 7, mode=mode, bootstrap=bootstrap)
    got = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, **kw)
    logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, return_logwt=True, **kw)
    assert np.array_equal(got["logz"], logz) and np.array_equal(got["information"], info)
    order = merge.merge_arrays(logl, birth, run_start)["order"]
    bound = n * 2.0 ** -52                    # a sequential fold of n subtractions from 1, each rounded once at magnitude <= 1
    worst = 0.0
    for s in range(5):
        fold = fip_oracle.accumulate([[None, (periods[order], np.exp(logwt[s]))]], [0.0, 1.0], nua, nub)[0]
        worst = max(worst, float(np.max(np.abs(fold - (1.0 - got["tip"][s])))))
    print("max |fold - (1 - tip)|", worst, "bound", bound)
    assert worst <= bound
    assert np.all((got["tip"] >= 0.0) & (got["tip"] <= 1.0)) and got["tip"].max() > 0.1


def test_union_counts_a_bin_once():
    logl, birth, run_start = _arrays(_ragged(4))
    n = logl.size
    _, nua, nub = _grid()
    one = _periods(n, 1, 5)
    kw = dict(nsamples=4, seed=9)
    single = fip.merged_tip_arrays(one, logl, birth, run_start, nua, nub, **kw)["tip"]
    twice = fip.merged_tip_arrays(np.concatenate([one, one], axis=1), logl, birth, run_start, nua, nub, **kw)["tip"]
    assert np.array_equal(single, twice)
    # two periods of a row inside one window: the row counts once in every bin of the joined span
    near = np.concatenate([one, one * (1.0 + 1e-9)], axis=1)
    both = fip.merged_tip_arrays(near, logl, birth, run_start, nua, nub, **kw)["tip"]
    assert np.max(np.abs(both - single)) < 1e-6 and both.max() <= 1.0
    beg, end = fip.row_intervals(near, nua, nub)
    assert np.all(beg[:, 1] == nua.size) and np.all(end[:, 1] == nua.size)       # one interval a row, the second slot unused
    # touching spans join, separate spans do not
    nua2, nub2 = np.arange(10.0), np.arange(10.0) + 1.0
    per = 2 * np.pi / np.array([[2.5, 3.5, 7.5], [7.5, 2.5, 2.6], [100.0, 4.5, 100.0]])
    beg, end = fip.row_intervals(per, nua2, nub2)
    assert beg.tolist() == [[2, 7, 10], [2, 7, 10], [4, 10, 10]] and end.tolist() == [[4, 8, 10], [3, 8, 10], [5, 10, 10]]


def test_tiling_windows_partition_the_weight():
    logl, birth, run_start = _arrays(_ragged(2))
    n = logl.size
    rng = np.random.default_rng(0)
    edges = np.linspace(0.05, 3.0, 201)
    nua, nub = edges[:-1].copy(), edges[1:].copy()
    omega = np.concatenate([rng.uniform(0.06, 0.9, n // 2), rng.uniform(2.0, 2.99, n - n // 2)])    # bins 58 .. 131 stay empty
    out = fip.merged_tip_arrays(2 * np.pi / omega, logl, birth, run_start, nua, nub, nsamples=16, seed=3)
    assert np.all(np.abs(out["tip"].sum(axis=1) - 1.0) <= 1e-12)
    hit = np.zeros(200, bool)
    hit[np.searchsorted(edges, omega, "right") - 1] = True
    assert (~hit).sum() > 50
    assert np.all(out["tip"][:, ~hit] == 0.0) and not np.signbit(out["tip"][:, ~hit]).any()


def test_expected_replicates_without_bootstrap_are_all_the_first():
    logl, birth, run_start = _arrays(_ragged(1))
    _, nua, nub = _grid()
    out = fip.merged_tip_arrays(_periods(logl.size, 2, 1), logl, birth, run_start, nua, nub, nsamples=6, seed=5,
                                mode="expected", bootstrap=False)
    assert all(np.array_equal(out[k][s], out[k][0]) for k in out for s in range(6))


def _results(seed, ncols):
    """The ragged runs as NestedResult with samples whose columns 1, 3, ... are periods."""
    runs = _ragged(seed)
    rng = np.random.default_rng(100 + seed)
    out = []
    for logl, birth in runs:
        samples = rng.normal(size=(len(logl), 2 * ncols + 1))
        samples[:, 1::2] = _periods(len(logl), ncols, int(rng.integers(1 << 30)))[:, :ncols] if ncols else samples[:, 1::2]
        out.append(NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=samples, logl=logl,
                                logwt=np.zeros_like(logl), logl_birth=birth))
    return out


def _shifted(results, shift):
    return [NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=r.samples, logl=r.logl + shift,
                         logwt=r.logwt, logl_birth=r.logl_birth + shift) for r in results]


def test_merged_fip_combines_the_models():
    models = [_results(0, 0), _results(1, 1), _results(2, 2)]
    cols = [[], [1], [1, 3]]
    nu, nua, nub = _grid()
    S = 23
    full = fip.merged_fip(models, cols, nua, nub, nsamples=S, seed=4, nu=nu, return_replicates=True)
    assert full["replicates"].shape == (S, nu.size) and np.array_equal(full["periods"], 2 * np.pi / nu)
    # model k is the standalone call with its own seed
    tips, logz = [], [merge.replicates(models[0], S, fip.model_seed(4, 0))[0]]
    for k in (1, 2):
        _, logl, birth, run_start = merge._stack(models[k])
        per = np.concatenate([r.samples[:, cols[k]] for r in models[k]])
        one = fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=S, seed=fip.model_seed(4, k))
        tips.append(one["tip"])
        logz.append(one["logz"])
    logz = np.stack(logz, axis=1)
    assert fip.model_seed(4, 1) == 4 + fip.MODEL_SEED_MUL and fip.MODEL_SEED_MUL % 2 == 1 and fip.MODEL_SEED_MUL < 2 ** 64
    assert np.array_equal(full["logz_replicates"], logz)
    pky = np.exp(logz - np.logaddexp.reduce(logz, axis=1)[:, None])
    assert np.allclose(full["pky_replicates"], pky, rtol=1e-13, atol=0) and np.allclose(pky.sum(axis=1), 1.0, atol=1e-14)
    want = 1.0 - pky[:, 1, None] * tips[0] - pky[:, 2, None] * tips[1]
    assert np.max(np.abs(full["replicates"] - want)) <= 1e-14
    # the statistics, accumulated block by block, are those of all replicates
    l10 = np.log10(np.maximum(full["replicates"], 1e-15))
    for step in (1, 5, 23):
        part = fip.merged_fip(models, cols, nua, nub, nsamples=S, seed=4, replicate_block=step)
        assert "replicates" not in part
        assert np.allclose(part["log10fip_err"], np.std(l10, axis=0), rtol=1e-9, atol=1e-15)
        assert np.array_equal(part["log10fip_min"], l10.min(axis=0)) and np.array_equal(part["log10fip_max"], l10.max(axis=0))
        assert np.array_equal(part["pky_err"], np.std(full["pky_replicates"], axis=0)) and np.array_equal(part["fip"], full["fip"])
        assert np.array_equal(part["logz_err"], np.std(logz, axis=0))
    # the point values are the expected weights' own
    point = fip.merged_fip(models, cols, nua, nub, nsamples=1, mode="expected", bootstrap=False, return_replicates=True)
    assert np.array_equal(point["replicates"][0], full["fip"]) and np.array_equal(point["pky"], full["pky"])
    assert np.array_equal(full["log10fip"], np.log10(np.maximum(full["fip"], 1e-15)))


def test_merged_fip_limits_of_the_null_model():
    m0, m1 = _results(0, 0), _results(1, 1)
    _, nua, nub = _grid()
    up = fip.merged_fip([_shifted(m0, 1000.0), m1], [[], [1]], nua, nub, nsamples=7, seed=1, return_replicates=True)
    assert np.all(up["replicates"] == 1.0) and np.all(up["fip"] == 1.0) and np.all(up["log10fip_err"] == 0.0)
    down = fip.merged_fip([_shifted(m0, -1000.0), m1], [[], [1]], nua, nub, nsamples=7, seed=1, return_replicates=True)
    _, logl, birth, run_start = merge._stack(m1)
    per = np.concatenate([r.samples[:, [1]] for r in m1])
    tip = fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=7, seed=fip.model_seed(1, 1))["tip"]
    assert np.array_equal(down["replicates"], 1.0 - tip)
    assert np.all(down["pky_replicates"][:, 1] == 1.0) and np.all(down["pky_err"] == 0.0)


def test_malformed_arguments_raise():
    logl, birth, run_start = _arrays(_ragged(0))
    n = logl.size
    _, nua, nub = _grid()
    good = _periods(n, 2, 0)

    def call(periods=good, nua=nua, nub=nub, **kw):
        return fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=2, **kw)

    call()
    bad = [dict(periods=np.ones((n, 9))), dict(periods=np.ones((n, 0))), dict(periods=good[:-1]), dict(nua=nua[::-1]),
           dict(nub=nub[::-1]), dict(nua=nua[:-1]), dict(nua=np.r_[nua[:-1], np.nan]), dict(mode="other"), dict(periods=np.ones((n, 2, 2)))]
    for value in (np.nan, np.inf, 0.0, -1.0):
        p = good.copy()
        p[n // 2, 1] = value
        bad.append(dict(periods=p))
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    m0, m1 = _results(0, 0), _results(1, 1)
    with pytest.raises(ValueError):
        fip.merged_fip([m0, m1], [[], [1], [1, 3]], nua, nub, nsamples=2)
    with pytest.raises(ValueError):
        fip.merged_fip([m0], [[]], nua, nub, nsamples=2)
    with pytest.raises(ValueError):
        fip.merged_fip([m0, m1], [[1], [1]], nua, nub, nsamples=2)


def test_the_library_exports_the_entry_within_abi_0_8():
    lib = _abi.load()
    assert hasattr(lib, "rvll_fip_replicates") and "rvll_fip_replicates" in _abi.PROTOTYPES
    major, minor = C.c_int32(), C.c_int32()
    lib.rvll_version(C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == (0, 8) == _abi.ABI_VERSION
    assert C.sizeof(_abi.FipMergedTiming) == 5 * 8 + 3 * 8 + 4 * 4
    assert fip.merged_table_bytes(1000, 3, 50) == 8 * 3000 + 8 * 50 + 8 * 4
