"""GP prediction on the device (rvll_celerite_predict_batch, correlated.CorrelatedNoiseModel.predict_batch, predictive.gp_bands)
against the dense definition in long double (predict_cases.dense_predict_reference) applied to the model's own residuals, at the
project's parity bound |delta| <= 1e-10 max(1, |reference|), every valid row of every output compared and NaN refused: every
composition of columns with Q on a different side of 1/2 from lane to lane and invalid rows between them, the band around
Q = 1/2 at sigma up to 100 svrad and a prior's decades (predict_cases lists the rows that are narrowed, each with the figure
that was measured outside the bound: the condition number, and the phases of the factor), every table size around the LDS
epoch tile and every query count around the transpose's tile, tables in time order (order = NULL), in decreasing time, all at one time and at a 30-second cadence.  Then what a wrong but plausible kernel
fails: log-L and flags are the log-L call's bits; a row's bits do not depend on the batch, the lane or the chunk; the epoch
outputs are in table order and the query outputs in the caller's order; invalid rows are NaN and leave their neighbours alone.

tests/test_predict_host.py shows that these shapes can tell the defects a sweep can have.  Every agreement case prints its
largest difference; profiles/celerite_predict_probe.txt records the largest seen."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import correlated_cases as cc
import predict_cases as pc
from evidence_amd import GpuRVModel, RvllError, _abi, correlated, predictive

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

B_MIXED = 130                                # two waves of rows and two more
NE_WIDE = 2 * cc.EPOCH_BLOCK + 1             # three epoch tiles, the last with one epoch
M_MAIN = 33
B_CASES = (1, 63, 64, 65, 130)
M_CASES = (0, 1, 31, 32, 33, 65)
CHUNK_CASES = (1, 64, 65)
ALONE = (0, 1, 2, 3, 4, 5, 6, 71)            # one row of every entry of cc.Q_SIDES and one of the second wave, none of them invalid
RANGES = {"offset": (-3.0, 3.0), "jitter": (0.5, 2.0), "k1": (1.0, 6.0), "period": (3.0, 80.0), "ecc": (0.0, 0.5),
          "omega": (0.0, 2 * np.pi), "ma0": (0.0, 2 * np.pi), "lin": (-2.0, 2.0), "fwhm": (-0.5, 0.5)}
PLANET_NAMES = [f"planet{n}_{s}" for n in (1, 2) for s in ("k1", "period", "ecc", "omega", "ma0")]
SUFFIXES = sorted({s for _, names in correlated.KINDS.values() for s in names})
TABLES = {f"ne{ne}": (lambda ne=ne: cc.make_table(ne)) for ne in cc.NE_CASES}
TABLES.update(cadence=cc.cadence_table, sorted=cc.sorted_table, decreasing=cc.decreasing_table, ties=cc.ties_table)


def make_model(table_id, planets=True, precision="fp64"):
    """Two planets with drift, a linear term and per-instrument jitter (or no planet) on a table, every parameter of gp1 to gp4
    free, so that one handle serves every composition."""
    table = TABLES[table_id]()
    ne = table.time.size
    names, fixed, linpar = [f"{i}_offset" for i in table.insts], {}, None
    if planets:
        names += PLANET_NAMES + [f"{i}_jitter" for i in table.insts] + ["drift_lin", "linpar_fwhm"]
        fixed = {"planet1_epoch": 55000.0, "planet2_epoch": 55001.5}
        linpar = {"fwhm": np.random.default_rng(ne).normal(0.0, 1.0, ne)}
    names += [f"gp{k}_{s}" for k in (1, 2, 3, 4) for s in SUFFIXES]
    return GpuRVModel(fixed, table, names, linpar_dict=linpar, precision=precision)


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(table_id, planets=True):
        if (table_id, planets) not in made:
            made[table_id, planets] = make_model(table_id, planets)
        return made[table_id, planets]
    yield get
    for m in made.values():
        m.close()


def make_theta(model, values, seed):
    n = len(next(iter(values.values())))
    rng = np.random.default_rng(seed)
    X = np.empty((n, model.ndim))
    for j, name in enumerate(model.parnames):
        X[:, j] = rng.uniform(*RANGES.get(name.split("_")[-1], (1.0, 2.0)), n)
    for name, v in values.items():
        X[:, model.parnames.index(name)] = v
    return X


def evaluate(label, model, terms, values, seed, m=M_MAIN):
    """The rows of a generator on a model: predict_batch with the variance against the long-double reference on the model's own
    residuals, log-L and flags against the log-L call's bits.  -> (gp, X, times, prediction, reference, valid)"""
    X = make_theta(model, values, seed)
    gp = correlated.CorrelatedNoiseModel(model, terms)
    res, var = model.residuals_batch(X)
    cols, valid = cc.rows_columns(terms, values)
    x = pc.query_times(model.table.time, m, seed)
    want = pc.dense_predict_reference(res, var, model.table.time, cols, x)
    assert np.array_equal(np.isfinite(np.asarray(want["mean_data"], dtype=np.float64)).all(axis=1), valid)
    pred = gp.predict_batch(X, x, return_var=True)
    pc.hold(label, pred, want, valid)
    assert np.array_equal(pred.residual[valid], res[valid]) and np.isnan(pred.residual[~valid]).all(), label
    logl, flags = gp.log_likelihood_batch(X, return_flags=True)
    assert np.array_equal(pred.logl, logl) and np.array_equal(pred.flags, flags), label
    assert not flags[valid].any() and (flags[~valid] == _abi.FLAG_NOISE_INVALID).all() and (logl[~valid] == -1e30).all(), label
    return gp, X, x, pred, want, valid


def same_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    """Every output of two predictions, on the given rows of each, bit for bit (NaN equal to NaN)."""
    for name in a._fields:
        u, v = getattr(a, name), getattr(b, name)
        if u is None or v is None:
            assert u is None and v is None, name
            continue
        assert np.array_equal(u[rows_a], v[rows_b], equal_nan=True), name


@pytest.mark.parametrize("composition", list(cc.COMPOSITIONS))
def test_lane_mixed_forms_and_batch_independence(gpu_required, models, composition):
    model = models("ne65")
    terms, values = cc.mixed_rows(composition, B_MIXED, seed=2, svmin=model.table.svrad.min())
    gp, X, x, pred, _, valid = evaluate(f"mixed {composition}", model, terms, values, seed=21)
    assert (~valid).sum() == B_MIXED // cc.INVALID_EVERY
    # the same rows alone, in smaller batches, reversed (another lane, another wave), and without the variance
    for i in ALONE:
        assert valid[i]
        same_bits(gp.predict_batch(X[i:i + 1], x, return_var=True), pred, rows_b=slice(i, i + 1))
    for b in B_CASES:
        same_bits(gp.predict_batch(X[:b], x, return_var=True), pred, rows_b=slice(0, b))
    back = gp.predict_batch(np.ascontiguousarray(X[::-1]), x, return_var=True)
    same_bits(back, pred, rows_a=slice(None, None, -1))
    shifted = gp.predict_batch(np.ascontiguousarray(X[7:]), x, return_var=True)
    same_bits(shifted, pred, rows_b=slice(7, None))
    plain = gp.predict_batch(X, x)
    assert plain.var is None and np.array_equal(plain.mean, pred.mean, equal_nan=True)
    # an invalid row leaves its neighbours alone: the batch with those rows repaired has the other rows' bits
    mended = X.copy()
    bad = np.flatnonzero(~valid)
    mended[bad] = X[bad - 1]
    again = gp.predict_batch(mended, x, return_var=True)
    same_bits(again, pred, rows_a=valid, rows_b=valid)
    same_bits(again, pred, rows_a=bad, rows_b=bad - 1)


@pytest.mark.parametrize("composition", ["sho", "rotation"])
def test_the_band_around_q_one_half(gpu_required, models, composition):
    for planets in (False, True):
        model = models("ne65", planets)
        # sigma up to 100 svrad; the sho band on the model with planets and jitter up to 30 (predict_cases: 2.5e-10 measured at 100)
        cap = pc.BAND_SHO_SIGMA_MAX_PLANETS if planets and composition == "sho" else None
        terms, values = pc.band_rows(model.table.svrad.min(), sho_sigma_max=cap)[composition]
        assert planets or values["gp1_sigma"].max() > 99.0 * model.table.svrad.min()
        *_, valid = evaluate(f"band {composition} planets {planets}", model, terms, values, seed=41)
        assert valid.all()


@pytest.mark.parametrize("composition", ["2", "12", "22", "211", "rotation"])
def test_the_priors_range(gpu_required, models, composition):
    model = models("ne65")
    terms, values = pc.wide_rows(composition, B_MIXED, seed=3, svmin=model.table.svrad.min())
    *_, valid = evaluate(f"wide {composition}", model, terms, values, seed=31)
    assert valid.all()


@pytest.mark.parametrize("table_id", list(TABLES))
def test_every_table_and_query_count(gpu_required, models, table_id):
    """One composition per J on every table, at every query count: the reference is taken once at the largest count, and every
    smaller count takes the first of those times, whose values do not depend on the others."""
    model = models(table_id, planets=False)
    ne = model.table.time.size
    for composition in ("1", "2", "111", "rotation"):
        terms, values = cc.mixed_rows(composition, 65, seed=5, svmin=model.table.svrad.min())
        gp, X, x, pred, want, valid = evaluate(f"{table_id} {composition} m {max(M_CASES)}", model, terms, values, seed=51, m=max(M_CASES))
        for m in M_CASES[:-1]:
            part = gp.predict_batch(X, x[:m], return_var=True)
            sub = dict(want, mean=want["mean"][:, :m], var=want["var"][:, :m])
            pc.hold(f"{table_id} {composition} m {m}", part, sub, valid)
            assert part.mean.shape == (65, m) and part.var.shape == (65, m)
            assert np.array_equal(part.mean_data, pred.mean_data, equal_nan=True) and np.array_equal(part.logl, pred.logl)
        none = gp.predict_batch(X)
        assert none.mean is None and none.var is None and np.array_equal(none.var_data, pred.var_data, equal_nan=True)
    if table_id == "sorted":                 # order = NULL is the identity, bit for bit
        assert np.array_equal(gp.order, np.arange(ne))
        out = [np.empty((65, ne)) for _ in range(3)] + [np.empty((65, x.size)) for _ in range(2)] + [np.empty(65), np.zeros(65, dtype=np.int32)]
        rc = model._lib.rvll_celerite_predict_batch(model._h, _abi.as_dp(X), 65, gp._terms_c, len(gp.terms), None, _abi.as_dp(x), x.size,
                                                    1, *[_abi.as_dp(a) for a in out[:6]], _abi.as_ip(out[6]), None)
        assert rc == _abi.OK
        same_bits(correlated.GpPrediction(*out), pred)
    if table_id == "decreasing":
        assert np.array_equal(gp.order, np.arange(ne)[::-1])


_CHILD = """
import sys
sys.path[:0] = {paths!r}
import numpy as np
import correlated_cases as cc, predict_cases as pc, test_gpu_predict as t
from evidence_amd import correlated
with t.make_model("ne65") as model:
    terms, values = cc.mixed_rows("211", t.B_MIXED, seed=2, svmin=model.table.svrad.min())
    X = t.make_theta(model, values, 21)
    x = pc.query_times(model.table.time, t.M_MAIN, 21)
    p = correlated.CorrelatedNoiseModel(model, terms).predict_batch(X, x, return_var=True)
np.savez({out!r}, **p._asdict())
"""


@pytest.mark.parametrize("chunk_rows", CHUNK_CASES)
def test_chunk_boundaries_in_a_fresh_process(gpu_required, models, tmp_path, chunk_rows):
    """RVLL_CELERITE_CHUNK_ROWS = 1, 64 and 65 cut 130 rows into 130, 3 and 2 chunks: the same bits as in one chunk."""
    model = models("ne65")
    terms, values = cc.mixed_rows("211", B_MIXED, seed=2, svmin=model.table.svrad.min())
    X = make_theta(model, values, 21)
    x = pc.query_times(model.table.time, M_MAIN, 21)
    whole = correlated.CorrelatedNoiseModel(model, terms).predict_batch(X, x, return_var=True)
    here = Path(__file__).resolve().parent
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ, RVLL_CELERITE_CHUNK_ROWS=str(chunk_rows))
    subprocess.run([sys.executable, "-c", _CHILD.format(paths=[str(here.parent), str(here)], out=out)], check=True, env=env, timeout=240)
    with np.load(out) as got:
        same_bits(correlated.GpPrediction(**{k: got[k] for k in got.files}), whole)


def test_layouts(gpu_required, models):
    """The epoch outputs are in table order on a table that is not in time order; the query outputs follow the caller's order."""
    model = models("ne65")
    assert not np.array_equal(np.argsort(model.table.time, kind="stable"), np.arange(NE_WIDE))
    terms, values = cc.mixed_rows("12", 65, seed=7, svmin=model.table.svrad.min())
    gp, X, x, pred, want, valid = evaluate("layouts", model, terms, values, seed=61)
    # the reference in time order would fail: the layout is not accidental
    order = np.argsort(model.table.time, kind="stable")
    assert cc.ref_err(pred.mean_data[valid], want["mean_data"][valid][:, order]).max() > 100 * cc.PARITY
    assert not np.array_equal(np.argsort(x, kind="stable"), np.arange(x.size))
    for perm in (np.argsort(x, kind="stable"), np.random.default_rng(3).permutation(x.size), np.arange(x.size)[::-1]):
        other = gp.predict_batch(X, np.ascontiguousarray(x[perm]), return_var=True)
        assert np.array_equal(other.mean, pred.mean[:, perm], equal_nan=True) and np.array_equal(other.var, pred.var[:, perm], equal_nan=True)
        assert np.array_equal(other.mean_data, pred.mean_data, equal_nan=True)
    # the series a user folds: the data minus the GP's mean at the epochs, for one theta
    i = int(np.flatnonzero(valid)[0])
    assert np.array_equal(gp.activity_corrected(X[i]), model.table.vrad - pred.mean_data[i])
    with pytest.raises(ValueError):
        gp.activity_corrected(X[int(np.flatnonzero(~valid)[0])])


def test_invalid_orbits_and_noise_between_valid_rows(gpu_required):
    ne = cc.EPOCH_BLOCK + 1
    table = cc.make_table(ne)
    names = ["a_offset", "b_offset", "planet1_k1", "planet1_period", "planet1_ecos", "planet1_esin", "planet1_ma0", "gp2_sigma",
             "gp2_rho", "gp2_q"]
    with GpuRVModel({"planet1_epoch": 55000.0}, table, names) as model:
        gp = correlated.CorrelatedNoiseModel(model, [("sho", "gp2")])
        ix = model.parnames.index
        X = make_theta(model, {"planet1_ecos": np.full(70, 0.1), "planet1_esin": np.full(70, 0.2), "gp2_sigma": np.full(70, 2.0),
                               "gp2_rho": np.full(70, 15.0), "gp2_q": np.full(70, 1.5)}, seed=2)
        x = pc.query_times(table.time, 31)
        good = gp.predict_batch(X, x, return_var=True)
        assert not good.flags.any() and all(np.isfinite(a).all() for a in good[:5])
        bad = X.copy()
        bad[3, ix("planet1_ecos")], bad[3, ix("planet1_esin")] = 0.8, 0.8        # ecos² + esin² > 1
        bad[10, ix("gp2_rho")] = 0.0
        bad[64, ix("gp2_q")] = -1.0
        bad[65, ix("gp2_sigma")] = np.nan
        bad[66, ix("planet1_ecos")], bad[66, ix("planet1_esin")], bad[66, ix("gp2_q")] = 0.8, 0.8, -1.0   # the orbit's flag alone
        got = gp.predict_batch(bad, x, return_var=True)
        hit = [3, 10, 64, 65, 66]
        assert (got.logl[hit] == -1e30).all()
        assert list(got.flags[hit]) == [_abi.FLAG_INVALID_ORBIT, _abi.FLAG_NOISE_INVALID, _abi.FLAG_NOISE_INVALID, _abi.FLAG_NOISE_INVALID,
                                        _abi.FLAG_INVALID_ORBIT]
        for a in got[:5]:
            assert np.isnan(a[hit]).all()
        rest = np.setdiff1d(np.arange(70), hit)
        same_bits(got, good, rows_a=rest, rows_b=rest)
        logl, flags = gp.log_likelihood_batch(bad, return_flags=True)
        assert np.array_equal(got.logl, logl) and np.array_equal(got.flags, flags)


def test_argument_errors(gpu_required, models):
    model = models("ne65")
    ne = NE_WIDE
    terms, values = cc.mixed_rows("2", 12, seed=2, svmin=model.table.svrad.min())
    X = make_theta(model, values, 1)
    gp = correlated.CorrelatedNoiseModel(model, terms)
    x = pc.query_times(model.table.time, 5)
    for wrong in (np.nan, np.inf, -np.inf):
        t = x.copy()
        t[2] = wrong
        with pytest.raises(RvllError) as err:
            gp.predict_batch(X, t)
        assert err.value.code == _abi.E_INVALID
    order = gp.order.copy()
    for wrong in (order[::-1].copy(), np.zeros(ne, dtype=np.int32), np.arange(ne, dtype=np.int32), order + 1):
        gp.order = np.ascontiguousarray(wrong, dtype=np.int32)
        with pytest.raises(RvllError) as err:
            gp.predict_batch(X, x)
        assert err.value.code == _abi.E_INVALID
    gp.order = order
    e3, q2 = [np.empty((12, ne)) for _ in range(3)], [np.empty((12, 5)) for _ in range(2)]
    logl, flags = np.empty(12), np.zeros(12, dtype=np.int32)

    def call(B=12, M=5, want_var=0, var=None, mean=q2[0], times=x, mean_data=e3[1]):
        return model._lib.rvll_celerite_predict_batch(
            model._h, _abi.as_dp(X), B, gp._terms_c, len(gp.terms), _abi.as_ip(order), None if times is None else _abi.as_dp(times), M,
            want_var, _abi.as_dp(e3[0]), None if mean_data is None else _abi.as_dp(mean_data), _abi.as_dp(e3[2]),
            None if mean is None else _abi.as_dp(mean), None if var is None else _abi.as_dp(var), _abi.as_dp(logl), _abi.as_ip(flags), None)
    assert call() == _abi.OK
    assert call(M=-1) == _abi.E_INVALID and call(B=-1) == _abi.E_INVALID
    assert call(var=q2[1]) == _abi.E_INVALID                                   # var without want_var
    assert call(want_var=1, var=q2[1]) == _abi.OK
    assert call(want_var=1) == _abi.E_INVALID                                  # want_var without var
    assert call(mean=None) == _abi.E_INVALID and call(times=None) == _abi.E_INVALID and call(mean_data=None) == _abi.E_INVALID
    assert call(M=0, times=None, mean=None) == _abi.OK
    with make_model("ne3", planets=False, precision="mixed") as mixed:
        gpm = correlated.CorrelatedNoiseModel(mixed, terms)
        with pytest.raises(RvllError) as err:
            gpm.predict_batch(make_theta(mixed, values, 1), x)
        assert err.value.code == _abi.E_UNSUPPORTED


def test_gp_bands(gpu_required, models):
    """64 draws: the band is bands_definition of the rows' means, total_sd the law of total variance over them."""
    model = models("ne65")
    terms, values = cc.mixed_rows("21", 64, seed=9, svmin=model.table.svrad.min())
    X = make_theta(model, values, 71)
    gp = correlated.CorrelatedNoiseModel(model, terms)
    x = np.sort(pc.query_times(model.table.time, M_MAIN, 5))
    pred = gp.predict_batch(X, x, return_var=True)
    ok = pred.flags == 0
    assert 0 < (~ok).sum() < 64
    out = predictive.gp_bands(gp, X, x)
    q, mean, nv = predictive.bands_definition(pred.mean[None], predictive.QUANTILES)
    assert np.array_equal(out["band"], q[0]) and np.array_equal(out["mean"], mean[0]) and np.array_equal(out["n_valid"], nv[0])
    assert (out["n_valid"] == ok.sum()).all() and out["band"].shape == (3, M_MAIN)
    want_sd = np.sqrt(pred.var[ok].mean(axis=0) + pred.mean[ok].var(axis=0))
    assert cc.rel_err(out["total_sd"], want_sd).max() <= 1e-12
    assert (out["band"][0] <= out["band"][1]).all() and (out["band"][1] <= out["band"][2]).all()
    bare = predictive.gp_bands(gp, X, x, quantiles=(0.5,), return_var=False)
    assert bare["total_sd"] is None and np.array_equal(bare["band"][0], out["band"][1])
