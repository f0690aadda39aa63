"""CPU: marginal histograms of merged runs (evidence_amd/marginals.py).  The numpy definition against an independent restatement
(np.histogram / np.histogram2d on the weights that merge.replicates_arrays returns) for both shrinkage modes with and without the
run bootstrap, on 3212 ragged rows with ties, plateaus and off-contour rows and a column built to sit on its edges; the Welford
statistics against np.mean / np.std / np.min / np.max; refusals; credible_levels on a Gaussian grid; marginals() under a
relabelling of the planets; the library exports the entry."""
import ctypes as C
import math

import numpy as np
import pytest

from evidence_amd import _abi, marginals, merge
from test_merge_host import _arrays, _ragged, _synthetic
from test_posterior_host import _columns, _result

EDGE_AXIS = np.array([-2.0, -1.5, -1.0, -0.25, 0.0, 0.5, 1.0, 1.75, 2.0])


def _small():
    """(logl, birth, run_start) of 3212 rows: the five ragged runs and two longer ones; over three 1024-row tiles, no multiple of
    any tile size."""
    rng = np.random.default_rng(7)
    runs = _ragged(5) + [_synthetic(rng, 40, 1500, kbatch=5, tie_grid=0.5), _synthetic(rng, 25, 1100, kbatch=1, off=3)]
    logl, birth, run_start = _arrays(runs)
    assert logl.size == 3212
    return logl, birth, run_start


def _edge_column(n):
    """Values that sit on the edges of EDGE_AXIS: every edge, its two neighbours in float64, -0.0 (an edge is 0.0), and values
    outside both ends; repeated to n rows."""
    e = EDGE_AXIS
    base = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), [e[0], e[-1], -0.0, 0.0, -3.0, 5.0, -2.5, 2.25]])
    return np.resize(base, n)


def _case(n):
    """values [n, 5] (the four columns of _columns and the edge column), the axes and the panels of the tests: a 1-D panel a
    column, one of 4096 bins, one of 1 bin, the 2-D panels (0, 1), (1, 2), (0, 4) and one of 64 x 64.  Two panel groups on the
    device."""
    values = np.concatenate([_columns(n, 5), _edge_column(n)[:, None]], axis=1)
    axes = [(0, np.linspace(-9.0, 9.0, 41)),
            (1, np.round(np.arange(0.0, 4.01, 0.1), 1)),                  # the column is rounded to 0.1: every value is an edge
            (2, 4.23 + np.linspace(-4e-5, 4e-5, 33)),
            (3, np.array([1234.0, 1234.5678, 1235.0, 1300.0])),           # the constant sits on an edge
            (4, EDGE_AXIS),
            (0, np.linspace(-10.0, 10.0, 4097)),
            (1, np.array([1.0, 3.0])),
            (0, np.linspace(-8.0, 8.0, 65)),
            (2, 4.23 + np.linspace(-3e-5, 3e-5, 65))]
    panels = [0, 1, 2, 3, 4, 5, 6, (0, 1), (1, 2), (0, 4), (7, 8)]
    return values, axes, panels


def _restated_counts(x, axes, panels):
    """Per panel the counts of np.histogram / np.histogram2d and the number of rows they leave out."""
    out = []
    for pan in panels:
        if isinstance(pan, int):
            col, edges = axes[pan]
            c = np.histogram(x[:, col], bins=edges)[0]
        else:
            (ca, ea), (cb, eb) = axes[pan[0]], axes[pan[1]]
            c = np.histogram2d(x[:, ca], x[:, cb], bins=(ea, eb))[0].astype(np.int64).reshape(-1)
        out.append((c, x.shape[0] - int(c.sum())))
    return out


def _restated_mass(x, axes, pan, p):
    if isinstance(pan, int):
        col, edges = axes[pan]
        return np.histogram(x[:, col], bins=edges, weights=p)[0] / p.sum()
    (ca, ea), (cb, eb) = axes[pan[0]], axes[pan[1]]
    return np.histogram2d(x[:, ca], x[:, cb], bins=(ea, eb), weights=p)[0].reshape(-1) / p.sum()


def test_the_edge_column_pins_the_binning_convention():
    x = _edge_column(64)
    got = marginals._axis_bins(x, EDGE_AXIS)
    e = EDGE_AXIS
    assert list(got[:9]) == [0, 1, 2, 3, 4, 5, 6, 7, 7]                  # an edge opens its bin; the last edge closes the last
    assert list(got[9:18]) == [0, 1, 2, 3, 4, 5, 6, 7, -1]               # just above
    assert list(got[18:27]) == [-1, 0, 1, 2, 3, 4, 5, 6, 7]              # just below
    assert list(got[27:35]) == [0, 7, 4, 4, -1, -1, -1, -1]              # -0.0 == +0.0
    assert e[4] == 0.0


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_the_definition_matches_an_independent_restatement(mode, bootstrap):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    S = 11
    kw = dict(seed=17, mode=mode, bootstrap=bootstrap)
    got = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=S, return_replicates=True, **kw)
    logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, S, return_logwt=True, **kw)
    assert np.array_equal(got["logz"], logz) and np.array_equal(got["information"], info)
    x = values[merge.merge_arrays(logl, birth, run_start)["order"]]
    start = got["panel_start"]
    assert got["counts"].dtype == np.int64 and got["outside_count"].dtype == np.int64
    assert start[-1] == got["counts"].size == 40 + 40 + 32 + 3 + 8 + 4096 + 1 + 1600 + 1280 + 320 + 4096
    assert got["mass"].shape == (S, start[-1]) and got["outside"].shape == (S, len(panels))
    restated = _restated_counts(x, axes, panels)
    for t, (c, out) in enumerate(restated):
        assert np.array_equal(got["counts"][start[t]:start[t + 1]], c), t
        assert got["outside_count"][t] == out, t
    assert got["outside_count"][4] > 0 and got["outside_count"][0] > 0 and got["outside_count"][3] == 0
    for s in range(S):
        with np.errstate(invalid="ignore"):
            p = np.exp(logwt[s])
        p = np.where(p > 0, p, 0.0)
        for t, pan in enumerate(panels):
            mass = got["mass"][s, start[t]:start[t + 1]]
            want = _restated_mass(x, axes, pan, p)
            nb = restated[t][0]
            assert np.all(np.abs(mass - want) <= 1e-12 + nb * 2.0 ** -61), (s, t)
            assert np.all(mass[nb == 0] == 0.0)
            total = math.fsum(mass) + got["outside"][s, t]
            assert abs(total - 1.0) <= 4 * 2.0 ** -53, (s, t, total - 1.0)
    m = got["mass"]
    # 1e-13 relative.  The mean is held to 1e-13 of itself.  np.std is itself only good to a few 2^-53 of the largest |x|: on
    # identical replicates (expected shrinkage, no bootstrap) np.mean is off by an ulp and np.std returns 4e-16 |x| where the
    # Welford update returns exactly 0.  So the std is held to 1e-13 of the largest mass of the bin over the replicates.
    assert np.allclose(got["mean"], np.mean(m, axis=0), rtol=1e-13, atol=0.0)
    assert np.all(np.abs(got["std"] - np.std(m, axis=0)) <= 1e-13 * np.max(m, axis=0))
    assert np.array_equal(got["min"], np.min(m, axis=0)) and np.array_equal(got["max"], np.max(m, axis=0))
    if mode == "expected" and not bootstrap:
        assert np.all(got["std"] == 0.0) and np.array_equal(got["min"], got["max"])


def test_blocked_evaluation_one_replicate_and_a_panel_alone_give_the_same_bits(monkeypatch):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    whole = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=7, seed=3, return_replicates=True)
    first = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=1, seed=3, return_replicates=True)
    alone = marginals.marginals_arrays(values, logl, birth, run_start, [axes[0], axes[4]], [(0, 1)], nsamples=7, seed=3,
                                       return_replicates=True)
    monkeypatch.setattr(marginals, "_BLOCK_ELEMS", 2 * logl.size)
    monkeypatch.setattr(merge, "_BLOCK_ELEMS", logl.size)
    blocked = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=7, seed=3, return_replicates=True)
    for key in whole:
        assert np.array_equal(whole[key], blocked[key], equal_nan=True), key
    assert np.array_equal(whole["mass"][0], first["mass"][0]) and np.array_equal(whole["mass"][0], first["mean"])
    lo, hi = whole["panel_start"][9:11]
    for key in ("mean", "std", "min", "max", "counts"):
        assert np.array_equal(whole[key][lo:hi], alone[key]), key
    assert np.array_equal(whole["mass"][:, lo:hi], alone["mass"]) and np.array_equal(whole["outside"][:, 9], alone["outside"][:, 0])


def test_a_replicate_of_empty_runs_is_nan_and_skipped():
    logl, birth, run_start, seed = _with_empty_runs()
    got = marginals.marginals_arrays(np.arange(3.0), logl, birth, run_start, [(0, [-1.0, 0.5, 3.0])], [0], nsamples=12, seed=seed,
                                     return_replicates=True)
    dead = np.isnan(got["mass"][:, 0])
    assert 0 < dead.sum() < 12 and np.array_equal(dead, np.isnan(got["outside"][:, 0]))
    assert np.array_equal(dead, np.isneginf(got["logz"]))
    assert np.array_equal(got["mean"], np.mean(got["mass"][~dead], axis=0)) or np.allclose(
        got["mean"], np.mean(got["mass"][~dead], axis=0), rtol=1e-13, atol=0)
    assert np.array_equal(got["max"], np.max(got["mass"][~dead], axis=0))


def _with_empty_runs():
    """A run of one row, a run of two and six empty runs: one bootstrap in ten draws the empty runs alone.  Returns the arrays
    and the first seed whose 12 replicates hold both kinds."""
    logl, birth = np.array([1.0, 0.5, 2.0]), np.array([-np.inf, -np.inf, 0.5])
    run_start = np.array([0, 1, 1, 1, 3, 3, 3, 3, 3], dtype=np.int64)
    for seed in range(200):
        logz, _ = merge.replicates_arrays(logl, birth, run_start, 12, seed=seed)
        if 0 < np.isneginf(logz).sum() < 12:
            return logl, birth, run_start, seed
    raise AssertionError("no seed found")


def test_refusals():
    logl, birth, run_start = _arrays(_ragged(4))
    n = logl.size
    values = _columns(n)
    good_axes, good_panels = [(0, [-1.0, 0.0, 1.0]), (1, [0.0, 2.0, 4.0])], [0, (0, 1)]

    def call(values=values, axes=good_axes, panels=good_panels, **kw):
        return marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=2, **kw)

    call()
    for bad in (np.nan, np.inf, -np.inf):
        v = values.copy()
        v[7, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            call(values=v)
        with pytest.raises(ValueError, match="edges"):
            call(axes=[(0, [-1.0, bad, 1.0])], panels=[0])
    with pytest.raises(ValueError, match="columns"):
        call(values=values[:, :0])
    with pytest.raises(ValueError, match="columns"):
        call(values=np.zeros((n, 65)))
    with pytest.raises(ValueError, match="rows"):
        call(values=values[:-1])
    with pytest.raises(ValueError, match="axes"):
        call(axes=[], panels=[0])
    with pytest.raises(ValueError, match="axes"):
        call(axes=[(0, [0.0, 1.0])] * 129, panels=[0])
    call(axes=[(0, [0.0, 1.0])] * 128, panels=[127])
    with pytest.raises(ValueError, match="panels"):
        call(panels=[])
    with pytest.raises(ValueError, match="panels"):
        call(panels=[0] * 257)
    call(panels=[0] * 256)
    for edges in ([0.0], [], np.linspace(0.0, 1.0, 4098), [0.0, 0.0, 1.0], [0.0, 1.0, 0.5]):
        with pytest.raises(ValueError, match="edges"):
            call(axes=[(0, edges)], panels=[0])
    call(axes=[(0, np.linspace(0.0, 1.0, 4097))], panels=[0])
    for col in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="column"):
            call(axes=[(col, [0.0, 1.0])], panels=[0])
    for pan in (2, -1, (0, 2), (0, -2), (0, 1, 1)):
        with pytest.raises(ValueError, match="panel"):
            call(panels=[pan])
    with pytest.raises(ValueError, match="bins"):
        call(axes=[(0, np.linspace(0.0, 1.0, 66)), (1, np.linspace(0.0, 1.0, 65))], panels=[(0, 1)])
    call(axes=[(0, np.linspace(0.0, 1.0, 65)), (1, np.linspace(0.0, 1.0, 65))], panels=[(0, 1)])
    with pytest.raises(ValueError, match="nsamples"):
        marginals.marginals_arrays(values, logl, birth, run_start, good_axes, good_panels, nsamples=0)
    with pytest.raises(ValueError, match="mode"):
        call(mode="mean")
    assert marginals.table_bytes(1000, 3) == 6000 and marginals.replicate_bytes(1000, 50, 2) == 8 * 1052


def test_credible_levels_on_a_gaussian_grid():
    g = np.linspace(-6.0, 6.0, 601)
    x, y = np.meshgrid(g, 0.5 * g, indexing="ij")                        # sigma_x = 1, sigma_y = 0.5
    dens = np.exp(-0.5 * (x ** 2 + (y / 0.5) ** 2))
    lv = marginals.credible_levels(dens)
    # the contour that holds 1 - exp(-r^2 / 2) of a 2-D Gaussian lies at the density peak * exp(-r^2 / 2): r = 1 and r = 2
    assert lv.shape == (2,) and lv[0] > lv[1]
    assert lv[0] == pytest.approx(np.exp(-0.5), rel=2e-3) and lv[1] == pytest.approx(np.exp(-2.0), rel=2e-2)
    for level, v in zip((0.393, 0.865), lv):
        inside = dens[dens >= v].sum() / dens.sum()
        above = dens[dens > v].sum() / dens.sum()
        assert above < level <= inside
    assert marginals.credible_levels([[1.0, 3.0], [0.0, 4.0]], levels=[0.5, 0.8, 0.9]).tolist() == [4.0, 3.0, 1.0]
    for bad in ([[0.0, 0.0]], [[1.0, -1.0]], [[np.nan, 1.0]]):
        with pytest.raises(ValueError):
            marginals.credible_levels(bad)
    with pytest.raises(ValueError):
        marginals.credible_levels([[1.0, 2.0]], levels=[1.0])


def test_marginals_does_not_depend_on_how_the_planets_are_labelled():
    runs = _ragged(2)
    rng = np.random.default_rng(5)
    names = ["offset", "planet1_period", "planet1_k1", "planet2_period", "planet2_k1"]
    results, swapped = [], []
    for l, b in runs:
        s = np.concatenate([rng.normal(size=(len(l), 1)), np.exp(rng.uniform(0, 3, (len(l), 4)))], axis=1)
        t = s.copy()
        pick = rng.random(len(l)) < 0.5
        t[np.ix_(pick, [1, 2, 3, 4])] = s[np.ix_(pick, [3, 4, 1, 2])]
        results.append(_result(s, l, b))
        swapped.append(_result(t, l, b))
    a = marginals.marginals(results, names, order=True, bins=12, nsamples=6, seed=4)
    b = marginals.marginals(swapped, names, order=True, bins=12, nsamples=6, seed=4)
    c = marginals.marginals(results, names, order=False, bins=12, nsamples=6, seed=4)
    assert len(a["panels"]) == 5 + 10 and a["names"] == names
    differs = False
    for pa, pb, pc in zip(a["panels"], b["panels"], c["panels"]):
        assert pa["columns"] == pb["columns"]
        for key in ("counts", "mass", "density", "density_err", "density_min", "density_max"):
            assert np.array_equal(pa[key], pb[key]), (pa["columns"], key)
        assert all(np.array_equal(ea, eb) for ea, eb in zip(pa["edges"], pb["edges"]))
        differs |= not np.array_equal(pa["counts"], pc["counts"])
    assert differs                                                       # the ordering did something
    period = a["panels"][1]
    assert period["columns"] == ("planet1_period",) and period["density"].shape == (12,)
    ratio = period["edges"][0][1:] / period["edges"][0][:-1]
    assert np.allclose(ratio, ratio[0], rtol=1e-9)                       # periods: logarithmic bins
    assert np.allclose(np.diff(a["panels"][0]["edges"][0]), np.diff(a["panels"][0]["edges"][0])[0], rtol=1e-9)
    pair = a["panels"][5]
    assert pair["columns"] == ("offset", "planet1_period") and pair["density"].shape == (12, 12)
    assert np.sum(period["density"] * np.diff(period["edges"][0])) + period["outside"] == pytest.approx(1.0, abs=1e-12)
    assert np.all(period["density_min"] <= period["density_max"]) and a["logz_err"] > 0
    only = marginals.marginals(results, names, columns=["planet2_k1"], bins=300, corner=False, nsamples=2)
    assert len(only["panels"]) == 1 and only["panels"][0]["counts"].shape == (300,)
    wide = marginals.marginals(results, names, columns=[0, 1], bins=100, nsamples=2)
    assert wide["panels"][2]["counts"].shape == (64, 64)


def test_the_library_exports_the_entry_within_abi_0_8():
    lib = _abi.load()
    assert hasattr(lib, "rvll_marginal_replicates") and "rvll_marginal_replicates" in _abi.PROTOTYPES
    major, minor = C.c_int32(), C.c_int32()
    lib.rvll_version(C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == (0, 8) == _abi.ABI_VERSION
    assert C.sizeof(_abi.MarginalTiming) == 5 * 8 + 3 * 8 + 4 * 4
    import evidence_amd
    assert evidence_amd.marginals is marginals and evidence_amd.marginals_arrays is marginals.marginals_arrays
    assert evidence_amd.credible_levels is marginals.credible_levels
