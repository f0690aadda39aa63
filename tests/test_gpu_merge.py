"""Merging runs on the device (rvll_merge_runs, rvll_merge_replicates; merge.merge / merge.replicates with device=0) against the
numpy definition of evidence_amd/merge.py: the ragged CPU cases (ties across runs, a -1e30 plateau, off-contour rows), a
resident 51 Peg ensemble of 16 runs, an input of over 2·10^6 rows, both shrinkage modes with and without the run bootstrap.
The order, the live counts and the off-contour count agree exactly; ln Z, H and the weights to round-off of the long running
sum.  Results are the same from call to call and in any batching of the replicates; malformed input is refused."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, merge, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from test_merge_host import _arrays, _ragged

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]


def _close(got, want, rel=1e-12):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))
    assert err.size == 0 or err.max() <= rel, float(err.max())


def _close_reps(got, want, rel=1e-12):
    for g, w in zip(got, want):
        _close(g, w, rel)


def test_merge_matches_the_definition(gpu_required):
    for seed in range(4):
        logl, birth, run_start = _arrays(_ragged(seed))
        want = merge.merge_arrays(logl, birth, run_start)
        timing = {}
        got = merge.merge_arrays(logl, birth, run_start, device=0, timing=timing)
        assert np.array_equal(got["order"], want["order"])
        assert np.array_equal(got["nlive_row"], want["nlive_row"])
        assert np.array_equal(got["run_index"], want["run_index"])
        assert got["off_contour"] == want["off_contour"] > 0
        _close(got["logz"], want["logz"])
        _close(got["information"], want["information"])
        _close(got["logwt"], want["logwt"])
        assert timing["rows"] == logl.size and timing["launches"] == 5 and timing["kernel_ms"] > 0


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_replicates_match_the_definition(gpu_required, mode, bootstrap):
    logl, birth, run_start = _arrays(_ragged(5))
    want = merge.replicates_arrays(logl, birth, run_start, 37, seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap,
                                   return_logwt=True)
    got = merge.replicates_arrays(logl, birth, run_start, 37, seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap,
                                  return_logwt=True, device=0)
    _close(got[0], want[0])
    _close(got[1], want[1])
    _close_reps(got[2], want[2])
    plain = merge.replicates_arrays(logl, birth, run_start, 37, seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap, device=0)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])
    if mode == "expected" and not bootstrap:
        one = merge.merge_arrays(logl, birth, run_start, device=0)
        assert np.all(got[0] == one["logz"]) and np.all(got[1] == one["information"])
        assert all(np.array_equal(row, one["logwt"]) for row in got[2])


def test_replicates_are_the_same_in_any_batching_and_from_call_to_call(gpu_required):
    logl, birth, run_start = _arrays(_ragged(6))
    one = merge.replicates_arrays(logl, birth, run_start, 9, seed=11, return_logwt=True, device=0)
    again = merge.replicates_arrays(logl, birth, run_start, 9, seed=11, return_logwt=True, device=0)
    timing = {}
    few = merge.replicates_arrays(logl, birth, run_start, 9, seed=11, return_logwt=True, device=0,
                                  block_bytes=2 * 8 * logl.size + 8, timing=timing)
    assert timing["launches"] == 4 + 5                      # setup (keys, two sorts, place), then 5 blocks of <= 2 replicates
    first = merge.replicates_arrays(logl, birth, run_start, 1, seed=11, return_logwt=True, device=0)
    for other in (again, few):
        assert all(np.array_equal(a, b) for a, b in zip(one, other))
    assert first[0][0] == one[0][0] and first[1][0] == one[1][0] and np.array_equal(first[2][0], one[2][0])


def _51peg():
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def test_51peg_resident_ensemble_merged(gpu_required):
    with _51peg() as m:
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, 17)), live=m, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
    assert all(g.logl_birth is not None for g in got)
    dev = merge.merge(got, device=0)
    ref = merge.merge(got)
    assert np.array_equal(dev.nlive_row, ref.nlive_row) and np.array_equal(dev.run_index, ref.run_index)
    assert np.array_equal(dev.logl, ref.logl) and np.array_equal(dev.samples, ref.samples)
    assert dev.nlive_row[0] == 16 * 400
    _close(dev.logz, ref.logz)
    _close(dev.information, ref.information)
    _close(dev.logwt, ref.logwt)
    for mode in ("random", "expected"):
        for bootstrap in (False, True):
            d = merge.replicates(got, nsamples=24, seed=7, mode=mode, bootstrap=bootstrap, device=0, return_logwt=True)
            r = merge.replicates(got, nsamples=3, seed=7, mode=mode, bootstrap=bootstrap, return_logwt=True)
            _close(d[0][:3], r[0])
            _close(d[1][:3], r[1])
            _close_reps(d[2][:3], r[2])
    # the merged ln Z sits among the runs', and the bootstrap error holds at least the shrinkage error
    singles = np.array([g.logz for g in got])
    assert singles.min() - 1.0 < dev.logz < singles.max() + 1.0
    boot = merge.logz_error(got, nsamples=200, device=0)
    shrink = merge.logz_error(got, nsamples=200, device=0, bootstrap=False)
    assert 0 < shrink < np.mean([g.logzerr for g in got]) and boot > 0.5 * shrink


def _big(n_runs=96, rows=22_000, seed=0):
    """Over 2·10^6 rows of arbitrary (logl, birth): ties on a grid, rows born at -inf, off-contour rows."""
    rng = np.random.default_rng(seed)
    n = n_runs * rows
    logl = np.round(rng.normal(-500.0, 40.0, n), 6)
    birth = logl - rng.exponential(30.0, n)
    birth[rng.random(n) < 0.02] = -np.inf
    off = rng.random(n) < 1e-4
    birth[off] = logl[off] + rng.integers(0, 2, off.sum())
    run_start = np.arange(0, n + 1, rows, dtype=np.int64)
    return logl, birth, run_start


def _wide(n_runs=96, rows=22_000, seed=0):
    """_big's recipe with a flat likelihood: log-L is N(0, 0.5) and births lie Exp(0.4) below, so the posterior mass is spread
    over the whole merged order (every row has a non-zero 62-bit weight in expected mode, no 1024-row tile holds more than 1 %;
    tests/test_merge_host.py asserts it) where _big's sits on its last rows.  A sum over rows that loses any part of the merged
    order is then off by far more than the 1e-10 bounds of the reducers' tests."""
    rng = np.random.default_rng(seed)
    n = n_runs * rows
    logl = np.round(rng.normal(0.0, 0.5, n), 6)
    birth = logl - rng.exponential(0.4, n)
    birth[rng.random(n) < 0.02] = -np.inf
    off = rng.random(n) < 1e-4
    birth[off] = logl[off] + rng.integers(0, 2, off.sum())
    run_start = np.arange(0, n + 1, rows, dtype=np.int64)
    return logl, birth, run_start


def test_two_million_rows_match_the_definition_on_the_first_replicates(gpu_required):
    logl, birth, run_start = _big()
    assert logl.size > 2_000_000
    want = merge.merge_arrays(logl, birth, run_start)
    got = merge.merge_arrays(logl, birth, run_start, device=0)
    assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["nlive_row"], want["nlive_row"])
    assert got["off_contour"] == want["off_contour"] > 0
    _close(got["logz"], want["logz"])
    _close(got["information"], want["information"])
    _close(got["logwt"], want["logwt"])
    for mode, bootstrap in (("random", True), ("random", False), ("expected", True)):
        timing = {}
        d = merge.replicates_arrays(logl, birth, run_start, 64, seed=3, mode=mode, bootstrap=bootstrap, device=0, timing=timing)
        r = merge.replicates_arrays(logl, birth, run_start, 2, seed=3, mode=mode, bootstrap=bootstrap)
        _close(d[0][:2], r[0])
        _close(d[1][:2], r[1])
        assert timing["elements"] == 64 * logl.size and timing["launches"] == 5


def _rel(got, want):
    """The largest error in _close's measure, for the record."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max())


def test_two_million_rows_of_spread_mass_match_the_definition_row_by_row(gpu_required):
    """_wide: rows of every weight throughout the merged order, so ln Z and H are sums to which the rows from 2^21 on (the
    second grid-stride pass of the 8192-block launches) contribute 8e-4 and no tile more than 0.3 %."""
    logl, birth, run_start = _wide()
    assert logl.size > 2 ** 21 + 8192
    want = merge.merge_arrays(logl, birth, run_start)
    got = merge.merge_arrays(logl, birth, run_start, device=0)
    assert np.array_equal(got["order"], want["order"]) and np.array_equal(got["nlive_row"], want["nlive_row"])
    assert got["off_contour"] == want["off_contour"] > 0
    print("max |logwt|", float(np.abs(want["logwt"][np.isfinite(want["logwt"])]).max()), " logz err / 1e-12",
          _rel(got["logz"], want["logz"]) / 1e-12, " information err / 1e-12", _rel(got["information"], want["information"]) / 1e-12,
          " logwt err / 1e-12", _rel(got["logwt"], want["logwt"]) / 1e-12)
    _close(got["logz"], want["logz"])
    _close(got["information"], want["information"])
    _close(got["logwt"], want["logwt"])
    for mode, bootstrap in (("random", True), ("random", False), ("expected", True)):
        timing = {}
        d = merge.replicates_arrays(logl, birth, run_start, 64, seed=3, mode=mode, bootstrap=bootstrap, device=0, timing=timing)
        r = merge.replicates_arrays(logl, birth, run_start, 2, seed=3, mode=mode, bootstrap=bootstrap)
        print(mode, bootstrap, "logz err / 1e-12", _rel(d[0][:2], r[0]) / 1e-12, " information err / 1e-12",
              _rel(d[1][:2], r[1]) / 1e-12)
        _close(d[0][:2], r[0])
        _close(d[1][:2], r[1])
        assert timing["elements"] == 64 * logl.size and timing["launches"] == 5


def test_oversize_weights_are_refused_with_nomem(gpu_required):
    logl, birth, run_start = _arrays(_ragged(7))
    with pytest.raises(RvllError) as exc:
        merge.replicates_arrays(logl, birth, run_start, 4, return_logwt=True, device=0, block_bytes=8 * logl.size - 8)
    assert exc.value.code == _abi.E_NOMEM
    merge.replicates_arrays(logl, birth, run_start, 4, return_logwt=True, device=0, block_bytes=8 * logl.size)


def _raw(logl, birth, run_start, nsamples=2, mode=0, bootstrap=1):
    """rvll_merge_replicates straight from ctypes, past the Python checks; returns the code."""
    lib = _abi.load()
    logl, birth = np.ascontiguousarray(logl, dtype=np.float64), np.ascontiguousarray(birth, dtype=np.float64)
    rs = np.ascontiguousarray(run_start, dtype=np.int64)
    out = np.zeros(2 * max(nsamples, 1))
    return lib.rvll_merge_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), logl.size, rs.ctypes.data_as(C.POINTER(C.c_int64)),
                                     len(rs) - 1, nsamples, mode, bootstrap, 0, _abi.as_dp(out), _abi.as_dp(out[out.size // 2:]),
                                     None, 0, None)


@pytest.mark.parametrize("args", [
    dict(logl=[0.0, np.nan, 1.0, 2.0]),
    dict(logl=[0.0, -np.inf, 1.0, 2.0]),
    dict(birth=[-np.inf, np.nan, 0.0, 0.0]),
    dict(run_start=[0, 3]),
    dict(run_start=[0, 3, 2, 4]),
    dict(nsamples=0),
    dict(mode=2),
    dict(bootstrap=2),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    kw = dict(logl=[0.0, 3.0, 1.0, 2.0], birth=[-np.inf, 0.5, 0.0, -np.inf], run_start=[0, 2, 4])
    kw.update(args)
    assert _raw(**kw) == _abi.E_INVALID
    assert _raw([0.0, 3.0, 1.0, 2.0], [-np.inf, 0.5, 0.0, -np.inf], [0, 2, 4]) == _abi.OK
