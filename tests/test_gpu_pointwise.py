"""Pointwise predictive checks on the device (rvll_pointwise_replicates; pointwise.pointwise_arrays / loo with device=0) against
the numpy definition of evidence_amd/pointwise.py: the ragged CPU cases for both shrinkage modes with and without the run
bootstrap, a constant unit, a run of more than one slab of rows, replicates without mass, a resident 51 Peg ensemble of 16 runs.
The bits are the same from call to call, in any batching of the replicates and in any split of the units; malformed input is
refused by the entry.

Bounds.  The merge tests hold every device weight to 1e-12 · max(1, |logwt|) of the definition's, and rows with |logwt| > 50
carry no mass, so any sum of non-negative terms is good to 5·10^-11 relative; DELTA = 1e-10 is twice that (tests/
test_gpu_posterior.py).  lpd and loo are logarithms of ratios of two such sums: 2 DELTA, and 2.5e-10 leaves room for the device's
exp and log.  With z = t - a and, from the definition's weights, S1 = sum p |z| / P, M1 = sum p z / P, M2 = sum p z^2 / P:
    |lpd err| <= 2.5e-10          |loo err| <= 2.5e-10
    |mean err| <= 1e-10 S1        |var err| <= 2e-10 (M2 + 2 |M1| S1)
None of them comes from a measurement; the largest ratios to the bounds are printed.  The comparison itself is
tests/pointwise_cases.py's compare (through check), shared with tests/test_gpu_pointwise_tiles.py, which takes the product across
every tile, slab and block edge."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import _abi, merge, pointwise, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from pointwise_cases import KEYS, check as _check
from test_gpu_merge import _51peg
from test_merge_host import _arrays, _ragged, _synthetic
from test_pointwise_host import _table

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_the_device_matches_the_definition(gpu_required, mode, bootstrap):
    """U = 7 gives 29 columns (a column tail), 37 replicates a replicate tail."""
    logl, birth, run_start = _arrays(_ragged(5))
    table = _table(logl, 5)
    kw = dict(seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap)
    timing = {}
    dev = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=37, device=0, timing=timing, **kw)
    _check(dev, table, logl, birth, run_start, 37, **kw)
    plain = merge.replicates_arrays(logl, birth, run_start, 37, device=0, **kw)
    assert np.array_equal(plain[0], dev["logz"]) and np.array_equal(plain[1], dev["information"])
    assert timing["rows"] == logl.size and timing["elements"] == 37 * logl.size and timing["blocks"] == 1
    assert timing["columns"] == 29 and timing["slabs"] == 1 and timing["unit_blocks"] == 1
    assert timing["launches"] == 5 + 4 and timing["kernel_ms"] > 0 and timing["threads"] == 256
    assert timing["kernel_ms"] == pytest.approx(timing["setup_ms"] + timing["weights_ms"] + timing["reduce_ms"], rel=1e-9)


def test_a_constant_unit_is_exact_and_loo_is_below_lpd(gpu_required):
    logl, birth, run_start = _arrays(_ragged(5))
    table = _table(logl, 5)
    # no row below the smallest value with weight: nothing is truncated, and the harmonic mean is below the arithmetic one
    table = np.maximum(table, pointwise.shifts_of(table, logl, birth, run_start)["shifts"][1])
    dev = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=12, seed=1, device=0)
    for key in ("lpd", "loo", "mean"):
        assert np.all(dev[key][:, 3] == -3.25), key
    assert np.all(dev["var"][:, 3] == 0.0)
    assert np.all(dev["truncated_rows"] == 0)
    assert np.all(dev["loo"] <= dev["lpd"])
    _check(dev, table, logl, birth, run_start, 12, seed=1)


def test_bits_are_stable_in_any_batching_and_from_call_to_call(gpu_required):
    logl, birth, run_start = _arrays(_ragged(6))
    table = _table(logl, 6)
    n, slab = logl.size, pointwise.slab_rows()
    kw = dict(nsamples=9, seed=11, device=0)
    one = pointwise.pointwise_arrays(table, logl, birth, run_start, **kw)
    again = pointwise.pointwise_arrays(table, logl, birth, run_start, **kw)
    timing = {}
    few = pointwise.pointwise_arrays(table, logl, birth, run_start, timing=timing, unit_block=7, **kw,
                                     block_bytes=pointwise.table_bytes(n, 7, slab) + 2 * pointwise.replicate_bytes(n, 7, slab) + 8)
    assert timing["blocks"] == 5 and timing["launches"] == 5 + 4 * 5
    first = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=1, seed=11, device=0)
    timing = {}
    split = pointwise.pointwise_arrays(table, logl, birth, run_start, unit_block=2, timing=timing, **kw)
    assert timing["unit_blocks"] == 4 and timing["columns"] == 3 * 9 + 5
    for key in one:
        assert np.array_equal(one[key], again[key], equal_nan=True), key
        assert np.array_equal(one[key], few[key], equal_nan=True), key
        assert np.array_equal(one[key], split[key], equal_nan=True), key
        if one[key].shape[0] == 9:
            assert np.array_equal(one[key][0], first[key][0], equal_nan=True), key
    # a unit's results do not depend on the units next to it
    alone = pointwise.pointwise_arrays(table[:, 4], logl, birth, run_start, **kw)
    for key in KEYS:
        assert np.array_equal(alone[key][:, 0], one[key][:, 4], equal_nan=True), key
    _check(one, table, logl, birth, run_start, 9, seed=11)


def test_more_than_one_slab_of_rows(gpu_required):
    """One run of slab + 333 rows: two slabs, the second a fraction of one, a row count that is no multiple of 4.  The run's mass
    sits at its end, so the test asks that the first slab still carries 1e-6 of it, four orders above the bounds."""
    slab = pointwise.slab_rows()
    rng = np.random.default_rng(12)
    logl, birth, run_start = _arrays([_synthetic(rng, 301, slab + 333 - 301, kbatch=1, off=6)])
    n = logl.size
    assert n > slab and n % slab != 0 and n % 4 != 0
    p = np.exp(merge.merge_arrays(logl, birth, run_start)["logwt"])
    assert 1e-6 < p[:slab].sum() < 1.0 - 1e-6
    table = _table(logl, 12)[:, [0, 2, 4]]
    kw = dict(seed=5, mode="random", bootstrap=False)
    timing = {}
    dev = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=16, device=0, timing=timing, **kw)
    assert timing["slabs"] == 2 and timing["columns"] == 13 and timing["rows"] == n
    _check(dev, table, logl, birth, run_start, 16, **kw)


def test_replicates_without_mass_are_nan(gpu_required):
    rng = np.random.default_rng(4)
    runs = [_synthetic(rng, 6, 30), (np.empty(0), np.empty(0)), (np.empty(0), np.empty(0))]
    logl, birth, run_start = _arrays(runs)
    table = _table(logl, 1)
    kw = dict(seed=3, mode="random", bootstrap=True)
    dev = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=40, device=0, **kw)
    empty = np.isneginf(dev["logz"])
    assert 0 < empty.sum() < 40
    for key in KEYS + ("waic",):
        assert np.all(np.isnan(dev[key][empty])) and np.all(np.isfinite(dev[key][~empty])), key
    _check(dev, table, logl, birth, run_start, 40, **kw)


def _raw(table, shifts=None, n_units=None, null=None, nsamples=2, mode=0, block_bytes=0):
    """rvll_pointwise_replicates straight from ctypes, past the Python checks, on a fixed four-row merge; returns the code."""
    lib = _abi.load()
    logl, birth = np.array([0.0, 3.0, 1.0, 2.0]), np.array([-np.inf, 0.5, 0.0, -np.inf])
    rs = np.array([0, 2, 4], dtype=np.int64)
    table = np.ascontiguousarray(table, dtype=np.float64)
    n_units = table.size // 4 if n_units is None else n_units
    width = max(n_units, 1)
    shifts = np.ascontiguousarray(np.zeros((3, width)) if shifts is None else shifts, dtype=np.float64)
    out = {k: np.zeros(nsamples * width + 1) for k in ("logz", "info", "lpd", "loo", "mean", "var")}
    ptr = {k: _abi.as_dp(v) for k, v in out.items()}
    ptr.update(table=_abi.as_dp(table), shifts=_abi.as_dp(shifts))
    if null:
        ptr[null] = None
    return lib.rvll_pointwise_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), 4, rs.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                         ptr["table"], n_units, ptr["shifts"], nsamples, mode, 1, 0, ptr["logz"], ptr["info"],
                                         ptr["lpd"], ptr["loo"], ptr["mean"], ptr["var"], block_bytes, None)


GOOD = [[-1.0, -2.0], [-3.0, -4.0], [-5.0, -6.0], [-7.0, -8.0]]


@pytest.mark.parametrize("args", [
    dict(table=[[-1.0, -2.0], [np.nan, -4.0], [-5.0, -6.0], [-7.0, -8.0]]),
    dict(table=[[-1.0, -2.0], [-3.0, -4.0], [-5.0, -np.inf], [-7.0, -8.0]]),
    dict(table=[[-1.0, -2.0], [-3.0, -4.0], [-5.0, -6.0], [2e30, -8.0]]),
    dict(table=[[-1.0, -2.0], [-3.0, -2e30], [-5.0, -6.0], [-7.0, -8.0]]),
    dict(table=GOOD, shifts=[[0.0, np.nan], [0.0, 0.0], [0.0, 0.0]]),
    dict(table=GOOD, shifts=[[0.0, 0.0], [0.0, 0.0], [2e30, 0.0]]),
    dict(table=GOOD, n_units=0),
    dict(table=GOOD, n_units=-1),
    dict(table=np.zeros((4, 4097))),
    dict(table=GOOD, null="table"),
    dict(table=GOOD, null="shifts"),
    dict(table=GOOD, null="lpd"),
    dict(table=GOOD, null="loo"),
    dict(table=GOOD, null="mean"),
    dict(table=GOOD, null="var"),
    dict(table=GOOD, null="logz"),
    dict(table=GOOD, mode=2),
    dict(table=GOOD, nsamples=0),
    dict(table=GOOD, block_bytes=-1),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    assert _raw(**args) == _abi.E_INVALID
    assert _raw(GOOD) == _abi.OK
    assert _raw([[-1e30, -2.0], [-3.0, -4.0], [-5.0, 1e30], [-7.0, -8.0]]) == _abi.OK


def test_a_block_bound_one_byte_short_is_refused_with_nomem(gpu_required):
    slab = pointwise.slab_rows()
    need = pointwise.table_bytes(4, 2, slab) + pointwise.replicate_bytes(4, 2, slab)
    assert _raw(GOOD, block_bytes=need - 1) == _abi.E_NOMEM and _raw(GOOD, block_bytes=need) == _abi.OK


def test_51peg_loo_from_a_resident_ensemble(gpu_required):
    with _51peg() as m:
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, 17)), live=m, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
        nights = pointwise.by_night(m.table.time)
        kw = dict(seed=7, mode="random", bootstrap=True)
        per_epoch = pointwise.loo(got, m, nsamples=64, device=0, **kw)
        per_night = pointwise.loo(got, m, nights, nsamples=64, device=0, **kw)
    _, logl, birth, run_start = pointwise._samples(got)
    assert per_epoch["units"] == m.table.time.shape[0] and per_night["units"] == nights.max() + 1 < per_epoch["units"]
    for res in (per_epoch, per_night):
        table = res["table"]
        valid = table[:, 0] > -1e29
        assert valid.sum() > 0.99 * valid.size
        assert np.all(np.abs(table[valid].sum(axis=1) - logl[valid]) <= 1e-9 * np.abs(logl[valid]))
        bound, ref = _check(res["replicates"], table, logl, birth, run_start, 8, unit_block=32, **kw)
        for key in KEYS:                                                  # the totals over the units
            err = np.abs(res["replicates"][key][:8].sum(axis=1) - ref[key].sum(axis=1))
            assert np.all(err <= bound[key].sum(axis=1)), key
        for key in ("lpd", "waic", "loo"):
            assert np.all(np.isfinite(res[key + "_err"])) and np.all(res[key + "_err"] > 0), key
            assert np.isfinite(res[key + "_total_err"]) and res[key + "_total_err"] > 0, key
            assert np.all(res[key + "_min"] <= res[key + "_max"])
        assert np.all(res["loo_ess"] > 1) and np.all(res["p_waic"] >= 0)
    # a night's log-likelihood is the sum of its epochs', so the totals of the in-sample density differ, the tables do not
    assert np.all(np.abs(per_night["table"].sum(axis=1) - per_epoch["table"].sum(axis=1))
                  <= 1e-12 * np.abs(per_epoch["table"].sum(axis=1)))
    cmp = pointwise.compare(per_epoch, per_epoch)
    assert cmp["elpd_diff"] == 0.0 and cmp["err_units"] == 0.0 and cmp["err_replicates"] > 0
    print("51 Peg k = 1: elpd_loo", per_epoch["loo_total"], "+/-", per_epoch["loo_total_err"], " p_waic", per_epoch["p_waic_total"],
          " per night:", per_night["loo_total"], "+/-", per_night["loo_total_err"])
