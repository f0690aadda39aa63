"""CPU: pointwise predictive checks of merged runs (evidence_amd/pointwise.py).  The numpy definition against a row-by-row
restatement in plain Python floats on the weights that merge.replicates_arrays returns, for both shrinkage modes with and without
the run bootstrap; the closed forms of a conjugate normal toy; the table of unit log-likelihoods on a model-shaped stub and the
two group builders; blocked evaluation gives the same bits; compare on hand-made results; the C prototype."""
import math
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from evidence_amd import _abi, merge, pointwise
from test_merge_host import _arrays, _ragged

UNITS = 7


def _table(logl, seed=0):
    """[n, 7]: a smooth unit, a tie-heavy one, one that follows log-L (and so the merged order), a constant, one with a heavy
    lower tail, one far from zero and one in which the rows of the -1e30 plateau are invalid orbits."""
    rng = np.random.default_rng(200 + seed)
    n = logl.size
    t = np.stack([-0.5 * rng.normal(0.0, 1.5, n) ** 2 - 1.0, np.round(rng.normal(-2.0, 0.5, n), 1), 0.01 * logl - 1.5,
                  np.full(n, -3.25), -np.exp(rng.normal(0.0, 1.2, n)), rng.normal(-900.0, 50.0, n), rng.normal(-4.0, 1.0, n)], axis=1)
    t[logl < -1e29, 6] = pointwise.INVALID
    return t


def _restated(table, logl, birth, run_start, logwt):
    """lpd, loo, mean and var [S, U] of the weights logwt [S, N], row by row in Python floats with exact sums (math.fsum), the
    variance about the replicate's own mean; and the shifts, loo_ess and truncated_rows."""
    m = merge.merge_arrays(logl, birth, run_start)
    t = table[m["order"]].tolist()
    ew = [float(x) for x in m["logwt"]]
    inside = [r for r, x in enumerate(ew) if x >= -43.0]
    n, units = len(t), len(t[0])
    shifts, ess, trunc = [], [], []
    for u in range(units):
        c = max(t[r][u] for r in inside)
        d = min(t[r][u] for r in inside)
        a = math.fsum(math.exp(ew[r]) * t[r][u] for r in inside) / math.fsum(math.exp(ew[r]) for r in inside)
        shifts.append((c, d, a))
        v = [math.exp(ew[r]) * math.exp(min(d - t[r][u], 0.0)) for r in inside]
        ess.append(math.fsum(v) ** 2 / math.fsum(x * x for x in v))
        trunc.append(sum(1 for r in range(n) if t[r][u] < d))
    out = {k: np.empty((len(logwt), units)) for k in ("lpd", "loo", "mean", "var", "s1", "m1", "m2")}
    for s, lw in enumerate(logwt):
        p = [math.exp(float(x)) if x > -math.inf else 0.0 for x in lw]
        P = math.fsum(p)
        for u, (c, d, a) in enumerate(shifts):
            col = [t[r][u] for r in range(n)]
            out["lpd"][s, u] = c + math.log(math.fsum(pr * math.exp(min(x - c, 0.0)) for pr, x in zip(p, col)) / P)
            out["loo"][s, u] = d - math.log(math.fsum(pr * math.exp(min(d - x, 0.0)) for pr, x in zip(p, col)) / P)
            mean = math.fsum(pr * x for pr, x in zip(p, col) if pr > 0.0) / P
            out["mean"][s, u] = mean
            out["var"][s, u] = math.fsum(pr * (x - mean) ** 2 for pr, x in zip(p, col) if pr > 0.0) / P
            out["s1"][s, u] = math.fsum(pr * abs(x - a) for pr, x in zip(p, col) if pr > 0.0) / P
            out["m1"][s, u] = abs(mean - a)
            out["m2"][s, u] = math.fsum(pr * (x - a) ** 2 for pr, x in zip(p, col) if pr > 0.0) / P
    return out, np.array(shifts).T, np.array(ess), np.array(trunc)


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_the_definition_matches_a_row_by_row_restatement(mode, bootstrap):
    """Bounds: a numpy sum of N <= 600 products is good to N 2^-53 < 1e-13 of the sum of their sizes; 1e-12 leaves room for the
    exp, the log and the division.  Every product is non-negative in lpd and loo, so their sums are good to 1e-12 relative and
    the logarithms to 1e-12 absolute; mean and var carry the sizes S1 = sum p |z| / P and M2 = sum p z^2 / P.  The restated
    variance is about the restated mean, whose own rounding (2^-52 relative, twice) enters it squared: the last term."""
    for seed in (0, 5):
        logl, birth, run_start = _arrays(_ragged(seed))
        table = _table(logl, seed)
        got = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=6, seed=17, mode=mode, bootstrap=bootstrap)
        logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, 6, seed=17, mode=mode, bootstrap=bootstrap,
                                                    return_logwt=True)
        assert np.array_equal(got["logz"], logz) and np.array_equal(got["information"], info)
        want, shifts, ess, trunc = _restated(table, logl, birth, run_start, logwt)
        for key in ("lpd", "loo", "mean", "var", "waic"):
            assert got[key].shape == (6, UNITS)
        assert np.array_equal(got["waic"], got["lpd"] - got["var"])
        assert np.array_equal(got["shifts"][:2], shifts[:2])
        assert np.all(np.abs(got["shifts"][2] - shifts[2]) <= 1e-12 * np.maximum(1.0, np.abs(shifts[2])))
        assert np.array_equal(got["truncated_rows"], trunc)
        assert np.all(np.abs(got["loo_ess"] - ess) <= 1e-10 * ess)
        assert np.all(np.abs(got["lpd"] - want["lpd"]) <= 1e-12 * np.maximum(1.0, np.abs(want["lpd"])))
        assert np.all(np.abs(got["loo"] - want["loo"]) <= 1e-12 * np.maximum(1.0, np.abs(want["loo"])))
        assert np.all(np.abs(got["mean"] - want["mean"]) <= 1e-12 * (want["s1"] + np.abs(want["mean"])))
        assert np.all(np.abs(got["var"] - want["var"]) <= 1e-12 * (want["m2"] + 2.0 * want["m1"] * want["s1"])
                      + (4e-16 * np.abs(want["mean"])) ** 2)
        # the constant unit: exactly the constant, no spread; no unit predicts held-out data better than its own
        assert np.all(got["lpd"][:, 3] == -3.25) and np.all(got["loo"][:, 3] == -3.25) and np.all(got["mean"][:, 3] == -3.25)
        assert np.all(got["var"][:, 3] == 0.0)
        assert np.all(got["loo"] <= got["lpd"] + 1e-12)


def test_a_replicate_without_mass_is_nan():
    rng = np.random.default_rng(4)
    from test_merge_host import _synthetic
    runs = [_synthetic(rng, 6, 30), (np.empty(0), np.empty(0)), (np.empty(0), np.empty(0))]
    logl, birth, run_start = _arrays(runs)
    table = _table(logl, 1)
    got = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=40, seed=3, bootstrap=True)
    empty = np.isneginf(got["logz"])
    assert 0 < empty.sum() < 40                             # (2/3)^3 of the replicates draw only empty runs
    for key in ("lpd", "loo", "mean", "var", "waic"):
        assert np.all(np.isnan(got[key][empty])) and np.all(np.isfinite(got[key][~empty]))


def _normal_logpdf(y, mu, var):
    return -0.5 * math.log(2.0 * math.pi * var) - 0.5 * (y - mu) ** 2 / var


def test_the_conjugate_normal_toy_has_its_closed_forms():
    """8 data y_i ~ N(mu, 1), one of them moved by 3, and 200 000 prior draws mu ~ U(-10, 10) as one run with every birth -inf:
    the posterior of mu is N(ybar, 1/8), so lpd_i = ln N(y_i; ybar, 1 + 1/8) and loo_i = ln N(y_i; ybar_-i, 1 + 1/7).  The bound
    is 3 / sqrt(ESS), ESS the Kish size of the expected weights: three standard errors of a weighted mean of quantities of order
    one.  The error is statistical and falls with the row count as the bound does, so it is the draw that is fixed here, not
    tuned rows: on this input ESS 12 356, bound 0.027, largest error 0.0037 for lpd and 0.0043 for loo (under a third of the
    bound), and six units have lpd - loo above twice the bound (0.07 to 1.03), so the bound tells the two apart."""
    rng = np.random.default_rng(2)
    y = rng.normal(0.7, 1.0, 8)
    y[2] += 3.0
    mu = rng.uniform(-10.0, 10.0, 200_000)
    table = -0.5 * math.log(2.0 * math.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2
    logl = table.sum(axis=1)
    birth = np.full(mu.size, -np.inf)
    run_start = np.array([0, mu.size])
    got = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=1, mode="expected", bootstrap=False)
    w = np.exp(merge.merge_arrays(logl, birth, run_start)["logwt"])
    ess = w.sum() ** 2 / (w * w).sum()
    bound = 3.0 / math.sqrt(ess)
    lpd = np.array([_normal_logpdf(y[i], y.mean(), 1.0 + 1.0 / 8.0) for i in range(8)])
    loo = np.array([_normal_logpdf(y[i], np.delete(y, i).mean(), 1.0 + 1.0 / 7.0) for i in range(8)])
    err_lpd, err_loo = np.abs(got["lpd"][0] - lpd).max(), np.abs(got["loo"][0] - loo).max()
    print("ESS", ess, "bound", bound, "max |lpd err|", err_lpd, "max |loo err|", err_loo, "lpd - loo", lpd - loo)
    assert 10_000 < ess < 16_000
    assert err_lpd <= bound and err_loo <= bound
    assert err_lpd <= bound / 3.0 and err_loo <= bound / 3.0       # the margin this input was found to have: see above
    assert np.count_nonzero(lpd - loo > 2.0 * bound) >= 4      # the bound tells the two apart
    assert np.all(got["truncated_rows"] > 0) and np.all(got["loo_ess"] > 1000)
    # WAIC agrees with LOO to the order of the squared corrections
    assert np.all(np.abs(got["waic"][0] - loo) <= bound + (lpd - loo) ** 2)


class _Stub:
    """A model-shaped object: a line with a jitter term over ten epochs of two instruments; a negative jitter is an invalid
    orbit."""

    def __init__(self):
        rng = np.random.default_rng(8)
        time = np.array([10.0, 10.1, 11.2, 10.3, 13.0, 11.25, 13.4, 20.0, 20.6, 19.9])
        self.table = SimpleNamespace(time=time, inst_id=np.array([0, 0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int32))
        self.y = rng.normal(0.0, 2.0, 10)
        self.sv = rng.uniform(0.5, 1.5, 10)

    def residuals_batch(self, X):
        X = np.atleast_2d(X)
        res = self.y[None, :] - X[:, 0:1] - X[:, 1:2] * (self.table.time[None, :] - 15.0)
        var = self.sv[None, :] ** 2 + X[:, 2:3] ** 2
        res[X[:, 2] < 0] = np.nan
        return res, np.broadcast_to(var, res.shape).copy()

    def loglike(self, X):
        res, var = self.residuals_batch(X)
        return np.array([-0.5 * len(r) * np.log(2 * np.pi) - np.sum(np.log(np.sqrt(v))) - np.sum(r ** 2 / (2 * v))
                         for r, v in zip(res, var)])


def test_unit_loglik_and_the_group_builders():
    m = _Stub()
    rng = np.random.default_rng(9)
    X = np.stack([rng.normal(0.0, 1.0, 50), rng.normal(0.0, 0.2, 50), rng.uniform(0.0, 1.0, 50)], axis=1)
    X[7, 2] = -1.0
    ok = np.arange(50) != 7
    t = pointwise.unit_loglik(m, X, chunk=16)
    assert t.shape == (50, 10) and np.all(t[7] == -1e30)
    want = m.loglike(X[ok])
    assert np.all(np.abs(t[ok].sum(axis=1) - want) <= 1e-12 * np.abs(want))
    assert np.array_equal(t, pointwise.unit_loglik(m, X))
    nights = pointwise.by_night(m.table.time)
    assert np.array_equal(nights, [0, 0, 1, 0, 2, 1, 2, 3, 4, 3])      # 13.0 and 13.4 are 0.4 d apart, 19.9 / 20.0 / 20.6 split
    assert np.array_equal(pointwise.by_night(m.table.time, gap=0.75), [0, 0, 1, 0, 2, 1, 2, 3, 3, 3])
    assert np.array_equal(pointwise.by_night([5.0]), [0])
    inst = pointwise.by_instrument(m)
    assert np.array_equal(inst, m.table.inst_id) and inst.dtype == np.int64
    for groups in (nights, inst):
        g = pointwise.unit_loglik(m, X, groups)
        assert g.shape == (50, groups.max() + 1) and np.all(g[7] == -1e30)
        for r in np.flatnonzero(ok)[:12]:
            sums = [0.0] * (groups.max() + 1)
            for e in range(10):                                           # left to right in rising epoch index
                sums[groups[e]] += float(t[r, e])
            assert g[r].tolist() == sums
    with pytest.raises(ValueError):
        pointwise.unit_loglik(m, X, np.array([0, 0, 2, 2, 2, 2, 2, 2, 2, 2]))
    with pytest.raises(ValueError):
        pointwise.unit_loglik(m, X, nights[:9])


def test_blocks_of_units_and_of_replicates_change_no_bit(monkeypatch):
    logl, birth, run_start = _arrays(_ragged(6))
    table = _table(logl, 6)
    kw = dict(nsamples=9, seed=11)
    one = pointwise.pointwise_arrays(table, logl, birth, run_start, **kw)
    for ub in (1, 2, 3, 100):
        got = pointwise.pointwise_arrays(table, logl, birth, run_start, unit_block=ub, **kw)
        for key in one:
            assert np.array_equal(one[key], got[key]), (ub, key)
    monkeypatch.setattr(pointwise, "_BLOCK_ELEMS", 2 * logl.size)
    monkeypatch.setattr(merge, "_BLOCK_ELEMS", 2 * logl.size)
    few = pointwise.pointwise_arrays(table, logl, birth, run_start, **kw)
    first = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=1, seed=11)
    alone = pointwise.pointwise_arrays(table[:, 4], logl, birth, run_start, **kw)
    for key in one:
        assert np.array_equal(one[key], few[key]), key
        if one[key].shape[0] == 9:
            assert np.array_equal(one[key][0], first[key][0]), key
    for key in ("lpd", "loo", "mean", "var", "waic"):
        assert np.array_equal(alone[key][:, 0], one[key][:, 4]), key
    with pytest.raises(ValueError):
        pointwise.pointwise_arrays(table, logl, birth, run_start, unit_block=0, **kw)


def test_refusals():
    logl, birth, run_start = _arrays(_ragged(7))
    table = _table(logl, 7)
    for bad in (np.nan, np.inf, -np.inf, 2e30, -2e30):
        t = table.copy()
        t[3, 2] = bad
        with pytest.raises(ValueError):
            pointwise.pointwise_arrays(t, logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError):
        pointwise.pointwise_arrays(table[:-1], logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError):
        pointwise.pointwise_arrays(table[:, :0], logl, birth, run_start, nsamples=2)
    with pytest.raises(ValueError):
        pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=2, mode="other")


def _made(loo, err):
    loo = np.asarray(loo, dtype=np.float64)
    return dict(units=loo.size, loo=loo, loo_total=float(loo.sum()), loo_total_err=err)


def test_compare_on_hand_made_results():
    a = _made([-1.0, -2.0, -3.0, -4.0], 0.3)
    b = _made([-1.5, -2.0, -4.5, -4.0], 0.4)
    c = pointwise.compare(a, b)
    assert c["elpd_diff"] == 2.0 and c["err_replicates"] == pytest.approx(0.5, rel=1e-15)
    assert np.array_equal(c["delta"], [0.5, 0.0, 1.5, 0.0])
    # U var(delta) = 4 * mean((delta - 0.5)^2) = 4 * (0 + 0.25 + 1 + 0.25) / 4
    assert c["err_units"] == pytest.approx(math.sqrt(1.5), rel=1e-15)
    back = pointwise.compare(b, a)
    assert back["elpd_diff"] == -2.0 and back["err_units"] == c["err_units"]
    with pytest.raises(ValueError):
        pointwise.compare(a, _made([-1.0], 0.1))


def test_the_prototype_is_declared():
    assert "rvll_pointwise_replicates" in _abi.PROTOTYPES and "rvll_pointwise_slab_rows" in _abi.PROTOTYPES
    assert len(_abi.PROTOTYPES["rvll_pointwise_replicates"][1]) == 21 and len(_abi.PROTOTYPES["rvll_pointwise_slab_rows"][1]) == 1
    assert _abi.ABI_VERSION == (0, 8)
    header = (Path(__file__).resolve().parents[1] / "include" / "rvll.h").read_text()
    assert "int rvll_pointwise_replicates(" in header and "int rvll_pointwise_slab_rows(" in header
    assert [name for name, _ in _abi.PointwiseTiming._fields_] == [
        "kernel_ms", "total_ms", "setup_ms", "weights_ms", "reduce_ms", "rows", "elements", "columns", "launches", "threads",
        "blocks", "slabs"]
    lib = _abi.load()
    assert hasattr(lib, "rvll_pointwise_replicates") and hasattr(lib, "rvll_pointwise_slab_rows")
    rows = pointwise.slab_rows()
    assert rows >= 64 and rows % 64 == 0
    assert pointwise.table_bytes(1000, 7, rows) == 8 * (1024 + 64 * -(-1000 // rows)) * 64
    assert pointwise.replicate_bytes(1000, 7, rows) == 8 * (1000 + -(-1000 // rows) * 64)
