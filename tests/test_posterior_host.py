"""CPU: posterior summaries of merged runs (evidence_amd/posterior.py).  The numpy definition against an independent
restatement (np.average, a weighted variance, np.quantile's inverted_cdf with weights) on the weights that
merge.replicates_arrays returns, for both shrinkage modes with and without the run bootstrap, on a tie-heavy column, a column
shaped like a period and a constant one; expected shrinkage without the bootstrap repeats the table's point estimate; the period
ordering of planets against a per-row loop; refusals; blocked evaluation gives the same bits."""
import numpy as np
import pytest

from evidence_amd import merge, posterior
from evidence_amd.nested import NestedResult
from test_merge_host import _arrays, _ragged


def _columns(n, seed=0):
    """[n, 4]: a smooth column, a tie-heavy one (rounded to 0.1), one shaped like a period, a constant."""
    rng = np.random.default_rng(100 + seed)
    return np.stack([rng.normal(0.0, 3.0, n), np.round(rng.normal(2.0, 0.5, n), 1), 4.23 + 1e-5 * rng.normal(size=n),
                     np.full(n, 1234.5678)], axis=1)


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_the_definition_matches_an_independent_restatement(mode, bootstrap):
    for seed in (0, 5):
        logl, birth, run_start = _arrays(_ragged(seed))
        values = _columns(logl.size, seed)
        q = (0.15865, 0.5, 0.84135, 0.01, 0.999)
        got = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=q, nsamples=11, seed=17, mode=mode,
                                         bootstrap=bootstrap)
        logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, 11, seed=17, mode=mode, bootstrap=bootstrap,
                                                    return_logwt=True)
        assert np.array_equal(got["logz"], logz) and np.array_equal(got["information"], info)
        x = values[merge.merge_arrays(logl, birth, run_start)["order"]]
        assert got["mean"].shape == (11, 4) and got["std"].shape == (11, 4) and got["quantiles"].shape == (11, 5, 4)
        for s in range(11):
            p = np.exp(logwt[s])
            assert p.sum() == pytest.approx(1.0, abs=1e-12)
            for c in range(4):
                mean = np.average(x[:, c], weights=p)
                std = np.sqrt(np.average((x[:, c] - mean) ** 2, weights=p))
                assert abs(got["mean"][s, c] - mean) <= 1e-13 * abs(mean)
                if c == 3:
                    assert got["std"][s, c] == 0.0 or got["std"][s, c] <= 1e-13 * abs(x[0, c])
                else:
                    assert abs(got["std"][s, c] - std) <= 1e-13 * std
                want = np.quantile(x[:, c], q, weights=p, method="inverted_cdf")
                assert np.array_equal(got["quantiles"][s, :, c], want)


def _result(samples, logl, birth):
    logl = np.asarray(logl, dtype=np.float64)
    return NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=np.asarray(samples), logl=logl,
                        logwt=np.zeros_like(logl), logl_birth=np.asarray(birth, dtype=np.float64))


def _results(seed=3):
    runs = _ragged(seed)
    rng = np.random.default_rng(seed)
    return [_result(_columns(len(l), seed + k)[:, :3] + rng.normal(), l, b) for k, (l, b) in enumerate(runs)]


def test_expected_replicates_without_the_bootstrap_repeat_the_point_estimate():
    results = _results()
    names = ["a", "b", "c"]
    got = posterior.summarize(results, nsamples=5, mode="expected", bootstrap=False)
    tab = posterior.table(results, names, nsamples=5, mode="expected", bootstrap=False)
    for s in range(5):
        assert np.array_equal(got["mean"][s], tab["mean"]) and np.array_equal(got["std"][s], tab["std"])
        assert np.array_equal(got["quantiles"][s], np.stack([tab["lower"], tab["median"], tab["upper"]]))
    for key in ("mean", "std", "median", "lower", "upper"):
        assert np.all(tab[key + "_err"] == 0.0)
    merged = merge.merge(results)
    assert tab["logz"] == merged.logz and tab["logz_err"] == 0.0
    assert tab["max_loglike"] == merged.logl[-1] and np.array_equal(tab["max_loglike_row"], merged.samples[-1])
    assert np.all(tab["lower"] <= tab["median"]) and np.all(tab["median"] <= tab["upper"])
    # with the bootstrap the replicates scatter, and the table carries that scatter as its errors
    boot = posterior.table(results, names, nsamples=40, seed=2)
    assert np.array_equal(boot["mean"], tab["mean"]) and np.all(boot["mean_err"] > 0) and boot["logz_err"] > 0
    assert "mean" in posterior.format_table(boot) and len(posterior.format_table(boot, other=tab).splitlines()) == 5


def test_summarize_selects_columns_and_appends_derived_ones():
    results = _results(4)
    names = ["a", "b", "c"]
    full = posterior.summarize(results, nsamples=3, seed=1)
    part = posterior.summarize(results, columns=["c", 0], parnames=names, derived=lambda s: s[:, 0] ** 2 + s[:, 1] ** 2,
                               nsamples=3, seed=1)
    assert part["mean"].shape == (3, 3)
    assert np.array_equal(part["mean"][:, 0], full["mean"][:, 2]) and np.array_equal(part["quantiles"][:, :, 1],
                                                                                     full["quantiles"][:, :, 0])
    tab = posterior.table(results, names, columns=["a"], derived=lambda s: s[:, :2] * 2.0, derived_names=["2a", "2b"], nsamples=3)
    assert tab["names"] == ["a", "2a", "2b"] and tab["mean"][1] == pytest.approx(2.0 * tab["mean"][0], rel=1e-12)
    with pytest.raises(ValueError, match="names"):
        posterior.table(results, names, derived=lambda s: s[:, 0], nsamples=2)


def _order_loop(samples, parnames):
    """Row by row: the planets' blocks re-dealt so that the periods rise; columns matched by position inside a block."""
    out = np.array(samples, dtype=float)
    blocks = []
    n = 1
    while any(name.startswith(f"planet{n}_") for name in parnames):
        blocks.append([i for i, name in enumerate(parnames) if name.startswith(f"planet{n}_")])
        n += 1
    pcol = [next(i for i in b if "period" in parnames[i]) for b in blocks]
    for r in range(out.shape[0]):
        row = samples[r]
        periods = [row[i] for i in pcol]
        if all(periods[k] <= periods[k + 1] for k in range(len(periods) - 1)):
            continue
        ranked = sorted(range(len(blocks)), key=lambda k: (periods[k], k))
        for slot, src in enumerate(ranked):
            for pos, col in enumerate(blocks[slot]):
                out[r, col] = row[blocks[src][pos]]
    return out


TWO = ["drift_lin", "planet1_period", "planet1_k1", "planet1_ecc", "planet1_omega", "inst_offset", "planet2_period",
       "planet2_k1", "planet2_secos", "planet2_sesin", "inst_jitter"]
THREE = ["planet1_k1", "planet1_period", "planet2_k1", "planet3_k1", "offset", "planet2_period", "planet3_period"]


@pytest.mark.parametrize("parnames", [TWO, THREE])
def test_order_planets_matches_a_row_loop(parnames):
    rng = np.random.default_rng(8)
    samples = rng.normal(size=(500, len(parnames)))
    pcols = [i for i, name in enumerate(parnames) if "period" in name]
    samples[:, pcols] = np.exp(rng.uniform(0.0, 5.0, (500, len(pcols))))
    samples[:50, pcols] = np.sort(samples[:50, pcols], axis=1)            # already ordered
    samples[50:80, pcols[1]] = samples[50:80, pcols[0]]                   # equal periods
    samples[80:90, pcols] = 3.0
    before = samples.copy()
    got = posterior.order_planets(samples, parnames)
    assert got is not samples and np.array_equal(samples, before)
    assert np.array_equal(got, _order_loop(samples, parnames))
    assert np.all(np.diff(got[:, pcols], axis=1) >= 0) and np.array_equal(got[:50], samples[:50])
    assert np.array_equal(got[80:90], samples[80:90])
    other = [i for i, name in enumerate(parnames) if not name.startswith("planet")]
    assert np.array_equal(got[:, other], samples[:, other])
    assert (got != samples).any()
    nplanets = len(pcols)
    blocks = [[i for i, name in enumerate(parnames) if name.startswith(f"planet{n + 1}_")] for n in range(nplanets)]
    for r in range(samples.shape[0]):                                     # every row keeps its planets, as whole blocks
        assert sorted(tuple(samples[r, b]) for b in blocks) == sorted(tuple(got[r, b]) for b in blocks)
    assert np.array_equal(posterior.order_planets(samples[:, :1], ["offset"]), samples[:, :1])
    with pytest.raises(ValueError):
        posterior.order_planets(samples, parnames[:-1])
    with pytest.raises(ValueError, match="same number"):
        posterior.order_planets(samples[:, :4], ["planet1_period", "planet1_k1", "planet2_period", "x"])


def test_summarize_orders_the_planets_first():
    runs = _ragged(2)
    rng = np.random.default_rng(5)
    names = ["planet1_period", "planet1_k1", "planet2_period", "planet2_k1"]
    results = [_result(np.exp(rng.uniform(0, 3, (len(l), 4))), l, b) for l, b in runs]
    ordered = [_result(posterior.order_planets(r.samples, names), r.logl, r.logl_birth) for r in results]
    a = posterior.summarize(results, order=True, parnames=names, nsamples=4)
    b = posterior.summarize(ordered, nsamples=4)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert np.all(a["mean"][:, 0] < a["mean"][:, 2])
    with pytest.raises(ValueError, match="parnames"):
        posterior.summarize(results, order=True)


def test_refusals():
    logl, birth, run_start = _arrays(_ragged(4))
    values = _columns(logl.size)
    for bad in (np.nan, np.inf, -np.inf):
        v = values.copy()
        v[7, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            posterior.summarize_arrays(v, logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError, match="columns"):
        posterior.summarize_arrays(values[:, :0], logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError, match="columns"):
        posterior.summarize_arrays(np.zeros((logl.size, 65)), logl, birth, run_start, nsamples=2)
    posterior.summarize_arrays(np.zeros((logl.size, 64)), logl, birth, run_start, nsamples=1, quantiles=[0.5])
    for q in (0.0, 1.0, -0.1, np.nan):
        with pytest.raises(ValueError, match="interval"):
            posterior.summarize_arrays(values, logl, birth, run_start, quantiles=[0.5, q], nsamples=2)
    with pytest.raises(ValueError, match="levels"):
        posterior.summarize_arrays(values, logl, birth, run_start, quantiles=np.linspace(0.1, 0.9, 17), nsamples=2)
    with pytest.raises(ValueError, match="levels"):
        posterior.summarize_arrays(values, logl, birth, run_start, quantiles=[], nsamples=2)
    posterior.summarize_arrays(values, logl, birth, run_start, quantiles=np.linspace(0.1, 0.9, 16), nsamples=1)
    with pytest.raises(ValueError, match="rows"):
        posterior.summarize_arrays(values[:-1], logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError, match="nsamples"):
        posterior.summarize_arrays(values, logl, birth, run_start, nsamples=0)
    with pytest.raises(ValueError, match="mode"):
        posterior.summarize_arrays(values, logl, birth, run_start, mode="mean")


def test_blocked_evaluation_gives_the_same_bits(monkeypatch):
    logl, birth, run_start = _arrays(_ragged(6))
    values = _columns(logl.size, 6)
    whole = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=9, seed=11)
    monkeypatch.setattr(posterior, "_BLOCK_ELEMS", 2 * logl.size)
    monkeypatch.setattr(merge, "_BLOCK_ELEMS", logl.size)
    blocked = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=9, seed=11)
    first = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=1, seed=11)
    for key in whole:
        assert np.array_equal(whole[key], blocked[key]), key
        assert np.array_equal(whole[key][0], first[key][0]), key
