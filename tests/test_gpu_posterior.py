"""Posterior summaries on the device (rvll_posterior_replicates; posterior.summarize_arrays / summarize / table with device=0)
against the numpy definition of evidence_amd/posterior.py: the ragged CPU cases for both shrinkage modes with and without the
run bootstrap, an input of over 2·10^6 rows, a resident 51 Peg ensemble of 16 runs.  The bits are the same from call to call
and in any batching; malformed input is refused by the entry.

Bounds.  The merge tests hold every device weight to 1e-12 · max(1, |logwt|) of the definition's, and rows with |logwt| > 50
carry no mass, so any partial sum of weights is good to 5·10^-11 relative; DELTA = 1e-10 is twice that.  With S1 = sum p |x| / P:
    |mean_dev - mean_def| <= 1e-10 S1
    |std_dev - std_def|   <= 1e-9 std_def + 1e-13 S1
    Q_def(q - DELTA) <= quantile_dev(q) <= Q_def(q + DELTA)
and on each test's own inputs at least 99 % of the brackets [Q_def(q - DELTA), Q_def(q + DELTA)] are one value, so the bracket
cannot hide a wrong answer."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import RvllError, _abi, merge, posterior, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from test_gpu_merge import _51peg, _big, _close, _wide
from test_merge_host import _arrays, _ragged
from test_posterior_host import _columns

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

DELTA = 1e-10
Q = posterior.QUANTILES


def _check(dev, values, logl, birth, run_start, nrep, **kw):
    """The first nrep replicates of the device result `dev` (levels Q) against the definition; returns (single, brackets)."""
    levels = np.array([[q - DELTA, q, q + DELTA] for q in Q]).reshape(-1)
    ref = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=levels, nsamples=nrep, **kw)
    s1 = posterior.summarize_arrays(np.abs(values), logl, birth, run_start, quantiles=[0.5], nsamples=nrep, **kw)["mean"]
    _close(dev["logz"][:nrep], ref["logz"])
    _close(dev["information"][:nrep], ref["information"])
    mean_err = np.abs(dev["mean"][:nrep] - ref["mean"])
    std_err = np.abs(dev["std"][:nrep] - ref["std"])
    print("max |mean err| / S1", float((mean_err / s1).max()), " max |std err| / (1e-9 std + 1e-13 S1)",
          float((std_err / (1e-9 * ref["std"] + 1e-13 * s1)).max()))
    assert np.all(mean_err <= 1e-10 * s1), float((mean_err / s1).max())
    assert np.all(std_err <= 1e-9 * ref["std"] + 1e-13 * s1), float((std_err / (1e-9 * ref["std"] + 1e-13 * s1)).max())
    lo, mid, hi = ref["quantiles"][:, 0::3], ref["quantiles"][:, 1::3], ref["quantiles"][:, 2::3]
    got = dev["quantiles"][:nrep]
    assert got.shape == lo.shape
    print("quantiles equal to the definition's:", int((got == mid).sum()), "of", got.size, " single brackets:",
          int((lo == hi).sum()))
    assert np.all((lo <= got) & (got <= hi))
    return int((lo == hi).sum()), lo.size


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_summaries_match_the_definition(gpu_required, mode, bootstrap):
    logl, birth, run_start = _arrays(_ragged(5))
    values = _columns(logl.size, 5)[:, :3]
    kw = dict(seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap)
    timing = {}
    dev = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=37, device=0, timing=timing, **kw)
    single, total = _check(dev, values, logl, birth, run_start, 37, **kw)
    assert total == 37 * 3 * 3 and single >= 0.99 * total
    plain = merge.replicates_arrays(logl, birth, run_start, 37, device=0, **kw)
    assert np.array_equal(plain[0], dev["logz"]) and np.array_equal(plain[1], dev["information"])
    assert timing["rows"] == logl.size and timing["elements"] == 37 * logl.size and timing["blocks"] == 1
    assert timing["launches"] == 5 + 2 * 3 + 3 and timing["kernel_ms"] > 0


def test_a_constant_column_has_no_spread(gpu_required):
    logl, birth, run_start = _arrays(_ragged(5))
    values = _columns(logl.size, 5)
    dev = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=12, seed=1, device=0)
    assert np.all(dev["mean"][:, 3] == values[0, 3]) and np.all(dev["std"][:, 3] == 0.0)
    assert np.all(dev["quantiles"][:, :, 3] == values[0, 3])
    _check(dev, values, logl, birth, run_start, 12, seed=1)


def test_bits_are_stable_in_any_batching_and_from_call_to_call(gpu_required):
    logl, birth, run_start = _arrays(_ragged(6))
    values = _columns(logl.size, 6)
    q = (0.02, 0.15865, 0.5, 0.84135, 0.98)
    one = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=q, nsamples=9, seed=11, device=0)
    again = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=q, nsamples=9, seed=11, device=0)
    timing = {}
    few = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=q, nsamples=9, seed=11, device=0, timing=timing,
                                     block_bytes=posterior.table_bytes(logl.size, 4) + 2 * 8 * logl.size + 8)
    assert timing["blocks"] == 5 and timing["launches"] == 5 + 2 * 4 + 3 * 5
    first = posterior.summarize_arrays(values, logl, birth, run_start, quantiles=q, nsamples=1, seed=11, device=0)
    for key in one:
        assert np.array_equal(one[key], again[key]), key
        assert np.array_equal(one[key], few[key]), key
        assert np.array_equal(one[key][0], first[key][0]), key
    # a column's results do not depend on the columns next to it
    alone = posterior.summarize_arrays(values[:, 2], logl, birth, run_start, quantiles=q, nsamples=9, seed=11, device=0)
    assert np.array_equal(alone["mean"][:, 0], one["mean"][:, 2]) and np.array_equal(alone["quantiles"][:, :, 0],
                                                                                     one["quantiles"][:, :, 2])


def test_two_million_rows_match_the_definition_on_the_first_replicates(gpu_required):
    logl, birth, run_start = _big()
    n = logl.size
    assert n > 2_000_000
    rng = np.random.default_rng(1)
    values = np.stack([rng.normal(0.0, 3.0, n), np.round(rng.normal(2.0, 0.5, n), 1), 4.23 + 1e-5 * rng.normal(size=n),
                       np.exp(rng.uniform(0.0, 7.0, n)), 0.01 * (logl + 500.0) + rng.normal(0.0, 0.1, n),
                       rng.integers(0, 5, n).astype(float)], axis=1)
    kw = dict(seed=3, mode="random", bootstrap=True)
    timing = {}
    dev = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=64, device=0, timing=timing, **kw)
    assert timing["elements"] == 64 * n and timing["rows"] == n
    print("timing", timing)
    single, total = _check(dev, values, logl, birth, run_start, 2, **kw)
    assert total == 2 * 3 * 6 and single >= 0.99 * total
    assert all(np.all(np.isfinite(dev[k])) for k in dev) and np.all(dev["std"] >= 0)
    assert np.all(np.diff(dev["quantiles"], axis=1) >= 0)


def test_two_million_rows_of_spread_mass_match_the_definition(gpu_required):
    """The same columns on _wide, whose mass covers the merged order (tests/test_merge_host.py): the means, deviations and
    quantiles are then sums to which every tile contributes, the rows from 2^21 on (the second grid-stride pass) 8e-4 of them,
    against bounds of 1e-10.  Column 4 follows log-L, and with it the merged order."""
    logl, birth, run_start = _wide()
    n = logl.size
    assert n > 2 ** 21 + 8192
    rng = np.random.default_rng(1)
    values = np.stack([rng.normal(0.0, 3.0, n), np.round(rng.normal(2.0, 0.5, n), 1), 4.23 + 1e-5 * rng.normal(size=n),
                       np.exp(rng.uniform(0.0, 7.0, n)), logl + rng.normal(0.0, 0.1, n),
                       rng.integers(0, 5, n).astype(float)], axis=1)
    kw = dict(seed=3, mode="random", bootstrap=True)
    timing = {}
    dev = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=8, device=0, timing=timing, **kw)
    assert timing["elements"] == 8 * n and timing["rows"] == n
    print("timing", timing)
    single, total = _check(dev, values, logl, birth, run_start, 2, **kw)
    assert total == 2 * 3 * 6 and single >= 0.99 * total
    assert all(np.all(np.isfinite(dev[k])) for k in dev) and np.all(dev["std"] >= 0)
    assert np.all(np.diff(dev["quantiles"], axis=1) >= 0)


def test_51peg_table_from_a_resident_ensemble(gpu_required):
    with _51peg() as m:
        names = list(m.parnames)
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, 17)), live=m, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
    dev = posterior.table(got, names, nsamples=200, seed=7, device=0)
    ref = posterior.table(got, names, nsamples=3, seed=7)
    _, cols, logl, birth, run_start = posterior._values(got, None, None, False, names)
    single, total = _check(dev["replicates"], cols, logl, birth, run_start, 3, seed=7)
    assert single >= 0.99 * total
    point = posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=1, mode="expected", bootstrap=False, device=0)
    _check(point, cols, logl, birth, run_start, 1, mode="expected", bootstrap=False)
    assert np.array_equal(point["mean"][0], dev["mean"]) and np.array_equal(point["quantiles"][0, 1], dev["median"])
    assert dev["max_loglike"] == ref["max_loglike"] and np.array_equal(dev["max_loglike_row"], ref["max_loglike_row"])
    _close(dev["logz"], ref["logz"])
    period = names.index("planet1_period")
    print(posterior.format_table(dev))
    assert 4.22 <= dev["median"][period] <= 4.24
    shrink = posterior.table(got, names, nsamples=200, seed=7, device=0, bootstrap=False)
    assert np.array_equal(shrink["mean"], dev["mean"])
    assert dev["mean_err"][period] > 0 and dev["mean_err"][period] >= 0.5 * shrink["mean_err"][period]


def _raw(values, quantiles=(0.5,), n_cols=None, n_q=None, block_bytes=0, null=None, nsamples=2):
    """rvll_posterior_replicates straight from ctypes, past the Python checks, on a fixed four-row merge; returns the code."""
    lib = _abi.load()
    logl, birth = np.array([0.0, 3.0, 1.0, 2.0]), np.array([-np.inf, 0.5, 0.0, -np.inf])
    rs = np.array([0, 2, 4], dtype=np.int64)
    values = np.ascontiguousarray(values, dtype=np.float64)
    q = np.ascontiguousarray(quantiles, dtype=np.float64)
    n_cols = values.size // 4 if n_cols is None else n_cols
    n_q = q.size if n_q is None else n_q
    out = {k: np.zeros(nsamples * max(n_cols, 1) * max(n_q, 1) + 1) for k in ("logz", "info", "mean", "sd", "quant")}
    ptr = {k: _abi.as_dp(v) for k, v in out.items()}
    ptr.update(values=_abi.as_dp(values), quantiles=_abi.as_dp(q))
    if null:
        ptr[null] = None
    return lib.rvll_posterior_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), 4, rs.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                         ptr["values"], n_cols, ptr["quantiles"], n_q, nsamples, 0, 1, 0, ptr["logz"],
                                         ptr["info"], ptr["mean"], ptr["sd"], ptr["quant"], block_bytes, None)


GOOD = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]


@pytest.mark.parametrize("args", [
    dict(values=[[1.0, 2.0], [np.nan, 4.0], [5.0, 6.0], [7.0, 8.0]]),
    dict(values=[[1.0, 2.0], [3.0, 4.0], [5.0, np.inf], [7.0, 8.0]]),
    dict(values=[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [-np.inf, 8.0]]),
    dict(values=GOOD, n_cols=0),
    dict(values=np.zeros((4, 65))),
    dict(values=GOOD, quantiles=[0.5, 0.0]),
    dict(values=GOOD, quantiles=[1.0]),
    dict(values=GOOD, quantiles=[-0.1]),
    dict(values=GOOD, quantiles=[np.nan]),
    dict(values=GOOD, quantiles=np.linspace(0.1, 0.9, 17)),
    dict(values=GOOD, n_q=0),
    dict(values=GOOD, null="values"),
    dict(values=GOOD, null="quantiles"),
    dict(values=GOOD, null="mean"),
    dict(values=GOOD, null="sd"),
    dict(values=GOOD, null="quant"),
    dict(values=GOOD, null="logz"),
    dict(values=GOOD, nsamples=0),
    dict(values=GOOD, block_bytes=-1),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    assert _raw(**args) == _abi.E_INVALID
    assert _raw(GOOD) == _abi.OK
    assert _raw(np.zeros((4, 64)), quantiles=np.linspace(0.1, 0.9, 16)) == _abi.OK


def test_what_merge_refuses_is_refused(gpu_required):
    logl, birth, run_start = _arrays(_ragged(7))
    values = _columns(logl.size, 7)
    lib = _abi.load()

    def call(logl=logl, birth=birth, rs=run_start, mode=0, bootstrap=1):
        out = [np.zeros(64) for _ in range(5)]
        q = np.array([0.5])
        return lib.rvll_posterior_replicates(0, _abi.as_dp(np.ascontiguousarray(logl)), _abi.as_dp(np.ascontiguousarray(birth)),
                                             len(logl), np.ascontiguousarray(rs).ctypes.data_as(C.POINTER(C.c_int64)), len(rs) - 1,
                                             _abi.as_dp(values), 4, _abi.as_dp(q), 1, 2, mode, bootstrap, 0,
                                             *[_abi.as_dp(o) for o in out], 0, None)

    bad_l, bad_b = logl.copy(), birth.copy()
    bad_l[3], bad_b[0] = np.nan, np.nan
    assert call() == _abi.OK
    assert call(logl=bad_l) == _abi.E_INVALID and call(birth=bad_b) == _abi.E_INVALID
    assert call(rs=np.r_[run_start[:-1], run_start[-1] - 1]) == _abi.E_INVALID
    assert call(mode=2) == _abi.E_INVALID and call(bootstrap=2) == _abi.E_INVALID


def test_a_block_bound_one_byte_short_is_refused_with_nomem(gpu_required):
    logl, birth, run_start = _arrays(_ragged(7))
    values = _columns(logl.size, 7)
    need = posterior.table_bytes(logl.size, 4) + 8 * logl.size
    with pytest.raises(RvllError) as exc:
        posterior.summarize_arrays(values, logl, birth, run_start, nsamples=4, device=0, block_bytes=need - 1)
    assert exc.value.code == _abi.E_NOMEM
    timing = {}
    exact = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=4, device=0, block_bytes=need, timing=timing)
    assert timing["blocks"] == 4
    roomy = posterior.summarize_arrays(values, logl, birth, run_start, nsamples=4, device=0)
    assert all(np.array_equal(exact[k], roomy[k]) for k in exact)
    assert _raw(GOOD, block_bytes=12 * 4 * 2 + 8 * 4 - 1) == _abi.E_NOMEM and _raw(GOOD, block_bytes=12 * 4 * 2 + 8 * 4) == _abi.OK
