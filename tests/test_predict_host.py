"""The GP prediction without a GPU: correlated.predict_dense (the definition in float64), correlated.predict_recursive (the
sweeps in numpy) and the host build of csrc/rvll_celerite_predict.h (the kernels' own source; tests/native/hostpredict.hip), each
against the dense definition in long double (predict_cases.dense_predict_reference) at the project's parity bound
|delta| <= 1e-10 max(1, |reference|), every valid row compared and NaN refused: every term case on every table size, rows whose
forms differ from row to row with invalid rows between them, the band around Q = 1/2 at sigma up to 100 svrad (30 for the
rotation rows far from 1/2: predict_cases), a prior's decades, and the tables in time order, in decreasing time, all at one
time and at a 30-second cadence; query times before, after, at and between the epochs, at both epochs of a tie, inside the 3000-day gap, duplicated and unsorted.  Then identities that need no
reference, and defects injected into the numpy sweeps, each of which must move an output by at least 100 bounds on the shapes the
GPU tests use: without that, the GPU tests could pass with the defect.

Every agreement case prints its largest difference.  Measured: the host build and predict_recursive differ by at most 3.4e-14
max(1, |value|) on the mixed rows and 2.7e-13 on the wide rows (both held to 1e-12), and in the band by what BAND_CLOSE lists;
predict_recursive against long double 2.3e-12 on the mixed rows, 9.3e-11 in the band at 100 svrad, 7.4e-11 on the wide rows."""
import subprocess

import numpy as np
import pytest

import correlated_cases as cc
import predict_cases as pc
from evidence_amd import _abi, correlated

HOST_NUMPY = 1e-12                           # the host build against predict_recursive: rounding, not the algorithm
NE_MAIN = cc.EPOCH_BLOCK + 1                 # 33 epochs: ties, the 3000-day gap, two epoch tiles


@pytest.fixture(scope="module")
def lib():
    built = pc.host_lib()
    if built is None:
        pytest.skip("no hipcc: the host build of csrc/rvll_celerite_predict.h cannot be made")
    return built


def _three_ways(lib, label, table, terms, values, seed, m=None, close=HOST_NUMPY, dense_rows=None):
    """The rows of a generator on a table, by the three implementations, each held to the long-double reference, and the host
    build to predict_recursive within `close` (a bound, or one a row).  dense_rows: the rows on which predict_dense is compared
    (all of them unless given).  -> (reference, recursive as a dict, valid)"""
    n = len(next(iter(values.values())))
    ne = table.time.size
    res, var = pc.synthetic_residuals(table, n, seed)
    cols, valid = cc.rows_columns(terms, values)
    x = pc.query_times(table.time, m, seed)
    want = pc.dense_predict_reference(res, var, table.time, cols, x)
    rec = [correlated.predict_recursive(res[i], var[i], table.time, cols[i], x) if valid[i] else None for i in range(n)]
    assert [p is not None for p in rec] == list(valid), label
    host = []
    for i in range(n):
        p, logl, flag = pc.host_predict(lib, terms, cc.row_values(values, i), res[i], var[i], table.time, x)
        assert (flag == 0) == bool(valid[i]), (label, i, flag)
        if flag:
            assert logl == correlated.INVALID_LOGL and flag == _abi.FLAG_NOISE_INVALID and p is None
        else:
            assert cc.rel_err(logl, correlated.log_likelihood_recursive(res[i], var[i], table.time, cols[i])) <= HOST_NUMPY
        host.append(p)
    rec_d, host_d = pc.stack(rec, ne, x.size), pc.stack(host, ne, x.size)
    pc.hold(f"{label} recursive", rec_d, want, valid)
    pc.hold(f"{label} host build", host_d, want, valid)
    pick = np.flatnonzero(valid if dense_rows is None else valid & dense_rows)
    den = [correlated.predict_dense(res[i], var[i], table.time, cols[i], x) for i in pick]
    pc.hold(f"{label} dense float64", pc.stack(den, ne, x.size), {k: v[pick] for k, v in want.items()}, np.ones(pick.size, dtype=bool))
    apart = np.zeros(n)
    for f in pc.FIELDS:
        apart[valid] = np.maximum(apart[valid], cc.rel_err(host_d[f][valid], rec_d[f][valid]).reshape(int(valid.sum()), -1).max(axis=1))
    bound = np.broadcast_to(np.asarray(close, dtype=np.float64), (n,))
    print(f"{label}: host build against predict_recursive {apart.max():.3e}, largest share of its bound {(apart / bound).max():.2f}")
    assert (apart <= bound).all(), (label, int(np.argmax(apart / bound)), apart.max())
    return want, rec_d, valid


def _one_row(values):
    return {k: np.array([float(v)]) for k, v in values.items()}


@pytest.mark.parametrize("ne", cc.NE_CASES)
@pytest.mark.parametrize("case", cc.TERM_CASES, ids=[c[0] for c in cc.TERM_CASES])
def test_term_cases_on_every_table_size(lib, case, ne):
    cid, terms, values = case
    _three_ways(lib, f"{cid} ne {ne}", cc.make_table(ne), terms, _one_row(values), seed=ne)


@pytest.mark.parametrize("composition", list(cc.COMPOSITIONS))
def test_mixed_rows(lib, composition):
    table = cc.make_table(NE_MAIN)
    terms, values = cc.mixed_rows(composition, 63, seed=2, svmin=table.svrad.min())
    _, _, valid = _three_ways(lib, f"mixed {composition}", table, terms, values, seed=1, m=25)
    assert (~valid).sum() == 63 // cc.INVALID_EVERY


# The host build against predict_recursive in the band, by sigma / svrad: two roundings of one algorithm drift apart as the
# condition number grows.  Measured on these rows 2.6e-13 up to 10 svrad, 5.3e-12 at 30 svrad, and at 100 svrad 1.05e-10 for sho
# and 7.0e-12 for the rotation rows in the pair basis; the bounds are four times those, except for sho at 100 svrad:
# the two bounds against the reference imply 2e-10 already, so that one is 1.5e-10, which still binds.
BAND_CLOSE = {"sho": ((10.0, HOST_NUMPY), (30.0, 2e-11), (100.0, 1.5e-10)), "rotation": ((10.0, HOST_NUMPY), (30.0, 2e-11), (100.0, 3e-11))}


@pytest.mark.parametrize("composition", ["sho", "rotation"])
def test_the_band_around_q_one_half(lib, composition):
    table = cc.make_table(NE_MAIN)
    sv = table.svrad.min()
    terms, values = pc.band_rows(sv)[composition]
    ratio = values["gp1_sigma"] / sv
    assert ratio.max() > 99.0                                             # the band at 100 svrad is in
    close = np.select([ratio <= r * 1.001 for r, _ in BAND_CLOSE[composition]], [b for _, b in BAND_CLOSE[composition]])
    _, _, valid = _three_ways(lib, f"band {composition}", table, terms, values, seed=1, m=25, close=close)
    assert valid.all()


@pytest.mark.parametrize("composition", ["2", "12", "22", "211", "rotation"])
def test_the_priors_range(lib, composition):
    table = cc.make_table(NE_MAIN)
    terms, values = pc.wide_rows(composition, 63, seed=3, svmin=table.svrad.min())
    _, _, valid = _three_ways(lib, f"wide {composition}", table, terms, values, seed=1, m=25,
                              dense_rows=pc.dense_comparable(values, table.svrad.min()))      # host against numpy: 2.7e-13 measured
    assert valid.all()


@pytest.mark.parametrize("table_id", ["sorted", "decreasing", "ties", "cadence"])
def test_the_other_tables(lib, table_id):
    table = {"sorted": cc.sorted_table, "decreasing": cc.decreasing_table, "ties": cc.ties_table, "cadence": cc.cadence_table}[table_id]()
    for composition in ("1", "2", "rotation"):
        terms, values = cc.mixed_rows(composition, 14, seed=6, svmin=table.svrad.min())
        _three_ways(lib, f"{table_id} {composition}", table, terms, values, seed=2)


def test_query_positions_and_order(lib):
    """No query, one query, and the special positions by name; the outputs come back in the order the times were given."""
    table = cc.make_table(NE_MAIN)
    terms, values = cc.TERM_CASES[6][1], _one_row(cc.TERM_CASES[6][2])          # sho + real
    res, var = pc.synthetic_residuals(table, 1, 3)
    cols, _ = cc.rows_columns(terms, values)
    s = np.sort(table.time)
    gap = int(np.argmax(np.diff(s)))
    tie = int(np.flatnonzero(np.diff(s) == 0.0)[0])
    assert s[gap + 1] - s[gap] > 2999.0
    named = np.array([s[0] - 2.0, s[-1] + 5.0, s[7], s[tie], s[tie + 1], s[gap] + 1500.0, s[gap] + 1500.0, s[0], s[-1], s[3] + 1e-9])
    for x in (None, np.empty(0), named[:1], named, named[::-1].copy(), named[np.random.default_rng(1).permutation(named.size)]):
        want = pc.dense_predict_reference(res, var, table.time, cols, x)
        rec = correlated.predict_recursive(res[0], var[0], table.time, cols[0], x)
        host, _, flag = pc.host_predict(lib, terms, cc.row_values(values, 0), res[0], var[0], table.time, x)
        assert flag == 0
        m = None if x is None else x.size
        for label, p in (("recursive", rec), ("host", host)):
            assert (p.mean is None) == (x is None)
            pc.hold(f"queries {m} {label}", pc.stack([p], NE_MAIN, m), want, np.array([True]))
    # the same times in another order give the same numbers in that order
    perm = np.random.default_rng(2).permutation(named.size)
    a, _, _ = pc.host_predict(lib, terms, cc.row_values(values, 0), res[0], var[0], table.time, named)
    b, _, _ = pc.host_predict(lib, terms, cc.row_values(values, 0), res[0], var[0], table.time, named[perm])
    assert np.array_equal(a.mean[perm], b.mean) and np.array_equal(a.var[perm], b.var)
    assert a.mean[5] == a.mean[6] and a.mean[3] == a.mean[4]                  # duplicates, and the two epochs of a tie


# ---- identities that need no reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("composition", ["1", "2", "12", "rotation"])
def test_identities(lib, composition):
    table = cc.make_table(NE_MAIN)
    terms, values = cc.mixed_rows(composition, 12, seed=8, svmin=table.svrad.min())           # row 12 would be the invalid one
    res, var = pc.synthetic_residuals(table, 12, 4)
    cols, valid = cc.rows_columns(terms, values)
    assert valid.all()
    for i in range(12):
        suma = float(cols[i][cols[i][:, 4] != correlated.FORM_SIN, 0].sum())
        for label in ("recursive", "host"):
            if label == "host":
                p, _, _ = pc.host_predict(lib, terms, cc.row_values(values, i), res[i], var[i], table.time, table.time)
            else:
                p = correlated.predict_recursive(res[i], var[i], table.time, cols[i], table.time)
            # the queries at the epochs give the values at the epochs
            assert cc.rel_err(p.mean, p.mean_data).max() <= cc.PARITY, (label, i)
            assert cc.rel_err(p.var, p.var_data).max() <= cc.PARITY, (label, i)
            slack = cc.PARITY * max(1.0, suma)
            assert (p.var >= -slack).all() and (p.var <= suma + slack).all(), (label, i)
            assert (p.var_data >= -slack).all() and (p.var_data <= suma + slack).all(), (label, i)


def test_sigma_zero_gives_no_signal(lib):
    table = cc.make_table(NE_MAIN)
    res, var = pc.synthetic_residuals(table, 1, 5)
    x = pc.query_times(table.time)
    for terms, values in (([("real", "gp1")], {"gp1_sigma": 0.0, "gp1_tau": 10.0}),
                          ([("sho", "gp1")], {"gp1_sigma": 0.0, "gp1_rho": 10.0, "gp1_q": 3.0}),
                          ([("sho", "gp1")], {"gp1_sigma": 0.0, "gp1_rho": 10.0, "gp1_q": 0.5 - 1e-6})):
        cols = cc.case_columns(terms, values)
        rec = correlated.predict_recursive(res[0], var[0], table.time, cols, x)
        host, _, flag = pc.host_predict(lib, terms, values, res[0], var[0], table.time, x)
        assert flag == 0
        for p in (rec, host):                    # 0 up to the rounding of r - var (r / var) and var - var² / var
            assert max(np.abs(a).max() for a in (p.mean_data, p.var_data, p.mean, p.var)) <= cc.PARITY
            assert not p.mean.any() and not p.var.any()
            assert cc.rel_err(p.alpha, res[0] / var[0]).max() <= cc.PARITY


def test_all_ties_closed_form(lib):
    """Every epoch at one time: Sigma = diag(var) + s 1 1^T with s = sum a, so by Sherman-Morrison
    alpha = r / var - (1 / var) s (sum r / var) / (1 + s sum 1 / var), and the GP at that time has mean s sum(alpha)."""
    table = cc.ties_table()
    res, var = pc.synthetic_residuals(table, 3, 6)
    for i, (terms, values) in enumerate((([("real", "gp1")], {"gp1_sigma": 2.0, "gp1_tau": 10.0}),
                                         ([("sho", "gp1")], {"gp1_sigma": 1.5, "gp1_rho": 10.0, "gp1_q": 0.5 + 1e-9}),
                                         ([("rotation", "gp1")], {"gp1_sigma": 2.5, "gp1_prot": 9.0, "gp1_q0": 1.0, "gp1_dq": 0.5, "gp1_mix": 0.3}))):
        cols = cc.case_columns(terms, values)
        s = float(cols[cols[:, 4] != correlated.FORM_SIN, 0].sum())
        alpha = res[i] / var[i] - (1.0 / var[i]) * s * (res[i] / var[i]).sum() / (1.0 + s * (1.0 / var[i]).sum())
        x = table.time[:1]
        rec = correlated.predict_recursive(res[i], var[i], table.time, cols, x)
        host, _, flag = pc.host_predict(lib, terms, values, res[i], var[i], table.time, x)
        assert flag == 0
        for p in (rec, host):
            assert cc.rel_err(p.alpha, alpha).max() <= cc.PARITY
            assert cc.rel_err(p.mean, s * alpha.sum()).max() <= cc.PARITY
            assert cc.rel_err(p.mean_data, s * alpha.sum()).max() <= cc.PARITY


# ---- the cases can tell: defects injected into the numpy sweeps -----------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ["drop_tie", "transpose", "last_g", "no_forward"])
def test_the_gpu_shapes_can_tell_a_defect(mutation):
    """On the GPU tests' shape (cc.make_table(65), 33 query times, a mixed composition with pair-basis rows) each defect moves
    some output of some row by at least 100 bounds."""
    table = cc.make_table(2 * cc.EPOCH_BLOCK + 1)
    terms, values = cc.mixed_rows("21", 12, seed=2, svmin=table.svrad.min())
    res, var = pc.synthetic_residuals(table, 12, 7)
    cols, valid = cc.rows_columns(terms, values)
    x = pc.query_times(table.time, 33)
    moved = 0.0
    for i in np.flatnonzero(valid):
        good = correlated.predict_recursive(res[i], var[i], table.time, cols[i], x)
        bad = correlated.predict_recursive(res[i], var[i], table.time, cols[i], x, mutate=mutation)
        if bad is None:
            moved = np.inf
            continue
        for f in pc.FIELDS:
            with np.errstate(invalid="ignore"):
                d = cc.rel_err(getattr(bad, f), getattr(good, f))
            moved = max(moved, float(np.nanmax(np.where(np.isnan(d), np.inf, d))))
    print(f"{mutation}: moves an output by {moved:.3e}")
    assert moved >= 100 * cc.PARITY, (mutation, moved)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_entry():
    assert "rvll_celerite_predict_batch" in _abi.PROTOTYPES
    assert len(_abi.PROTOTYPES["rvll_celerite_predict_batch"][1]) == 17
    assert _abi.ABI_VERSION == (0, 8)
    header = (cc.HERE.parent / "include" / "rvll.h").read_text()
    assert "int rvll_celerite_predict_batch(" in header
    if not _abi.LIB_PATH.exists():
        pytest.skip("librvll.so has not been built")
    out = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert " T rvll_celerite_predict_batch" in out
