"""Equal-weight draws on the device (rvll_draw_replicates; draws.draw_arrays with device=0) against the numpy definition of
evidence_amd/draws.py, on the 3212 ragged rows of the marginal tests (over three 1024-row tiles of the running sum; ties, plateaus
and off-contour rows) for both shrinkage modes with and without the run bootstrap and 1, 64 and 1000 draws; and on 528 000 rows
whose mass covers the merged order (_wide of tests/test_gpu_merge.py: 516 tiles, three steps of the scan of the tile sums).

Exact.  With the device's own integers m (the optional output `fixed`) the definition's pick must give the device's rows bit for
bit: every decision is an integer comparison.  ln Z and H are rvll_merge_replicates' bits.

Against the definition's weights.  The merge tests hold every device weight to 1e-12 · max(1, |logwt|) of the definition's, and
rows with |logwt| > 50 carry no mass, so any partial sum of weights is good to 5·10^-11 relative; 1e-10 is twice that, and each
row is rounded to a multiple of 2^-62 (tests/test_gpu_marginals.py):  |C_dev[i] - C_def[i]| <= 1e-10 C_def[i] + (i + 1).  A draw's
threshold tau = k Q + O moves by at most the bound of M (Q and O are fractions of M), and a boundary C_i by its own, so a draw
whose tau lies within 4·10^-10 M + (N + 1) units of a boundary of C may land on the neighbouring row: it is fragile.  Every other
draw must equal the definition's, and at most 1 in 1000 of the draws compared may be fragile."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import RvllError, _abi, draws, marginals, merge
from evidence_amd.shrinkage import replicate_seeds
from test_gpu_marginals import _check, _reference
from test_gpu_merge import _wide
from test_marginals_host import _case, _small
from test_merge_host import _arrays, _ragged, _synthetic

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

_I64 = C.POINTER(C.c_int64)
S = 24
SEED = 2 ** 64 - 3
_REFS = {}


def _definition_weights(mode, bootstrap):
    """(order, m [S, N], logz, info) of the definition on the small input: computed once, shared, never changed."""
    key = (mode, bootstrap)
    if key not in _REFS:
        logl, birth, run_start = _small()
        logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, S, seed=SEED, mode=mode, bootstrap=bootstrap,
                                                    return_logwt=True)
        out = (merge._layout(logl, birth, run_start)["order"].astype(np.int64), draws.fixed_point(logwt), logz, info)
        for v in out:
            v.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _own(order, fixed, seeds, n):
    """The definition's pick applied to the integers `fixed` [S, N]."""
    out = np.empty((fixed.shape[0], n), np.int64)
    for s in range(fixed.shape[0]):
        i = draws.pick(fixed[s], seeds[s], n)
        out[s] = np.where(i >= 0, order[np.maximum(i, 0)], -1)
    return out


def _fragile(c, seed_s, n):
    """bool [n]: the draws of the replicate with the definition's running sum c [N] whose threshold lies within
    4e-10 M + (N + 1) units of a boundary of c (the module's docstring)."""
    M, N = int(c[-1]), c.shape[0]
    tau = draws.thresholds(M, seed_s, n)
    j = np.searchsorted(c, tau, side="right")
    near = np.minimum(np.abs(c[j] - tau), np.abs(tau - c[np.maximum(j - 1, 0)]))
    return near <= 4e-10 * M + (N + 1)


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_rows_are_the_definition_on_the_devices_own_integers_and_close_to_the_definitions(gpu_required, mode, bootstrap):
    logl, birth, run_start = _small()
    N = logl.size
    order, m_def, logz_def, _ = _definition_weights(mode, bootstrap)
    seeds = replicate_seeds(SEED, S)
    plain = merge.replicates_arrays(logl, birth, run_start, S, seed=SEED, mode=mode, bootstrap=bootstrap, device=0)
    compared = fragile = 0
    for n in (1, 64, 1000):
        rows, logz, info, fixed, msum = draws.device_integers(logl, birth, run_start, n, S, seed=SEED, mode=mode,
                                                              bootstrap=bootstrap)
        assert np.array_equal(plain[0], logz) and np.array_equal(plain[1], info)
        assert np.array_equal(msum, fixed.sum(axis=1, dtype=np.int64)) and fixed.min() >= 0
        assert np.array_equal(rows, _own(order, fixed, seeds, n)), n
        via = draws.draw_arrays(logl, birth, run_start, n, S, seed=SEED, mode=mode, bootstrap=bootstrap, device=0)
        assert np.array_equal(via[0], rows) and np.array_equal(via[1], logz)
        # the definition's weights
        c_dev, c_def = np.cumsum(fixed, axis=1, dtype=np.int64), np.cumsum(m_def, axis=1, dtype=np.int64)
        bound = 1e-10 * c_def.astype(np.float64) + np.arange(1, N + 1)
        err = np.abs(c_dev - c_def)
        print("n", n, "max |C err| / bound", float((err / bound).max()))
        assert np.all(err <= bound)
        want = _own(order, m_def, seeds, n)
        for s in range(S):
            frag = _fragile(c_def[s], seeds[s], n)
            assert np.array_equal(rows[s][~frag], want[s][~frag]), (n, s)
            compared += n
            fragile += int(frag.sum())
    print("fragile draws", fragile, "of", compared)
    assert fragile * 1000 <= compared


def test_bits_do_not_depend_on_the_batching_or_on_the_other_replicates(gpu_required):
    logl, birth, run_start = _small()
    kw = dict(seed=11, device=0)
    timing = {}
    one = draws.draw_arrays(logl, birth, run_start, 64, 9, timing=timing, **kw)
    assert timing["blocks"] == 1 and timing["launches"] == 4 + 6 and timing["tiles"] == 4 and timing["draws"] == 9 * 64
    assert timing["rows"] == logl.size and timing["kernel_ms"] > 0
    again = draws.draw_arrays(logl, birth, run_start, 64, 9, **kw)
    few = draws.draw_arrays(logl, birth, run_start, 64, 9, block_bytes=8 * logl.size * 3 + 8, timing=timing, **kw)
    assert timing["blocks"] == 3 and timing["launches"] == 4 + 6 * 3
    single = draws.draw_arrays(logl, birth, run_start, 64, 9, block_bytes=8 * logl.size, timing=timing, **kw)
    assert timing["blocks"] == 9
    first = draws.draw_arrays(logl, birth, run_start, 64, 1, **kw)
    for a, b, c, d in zip(one, again, few, single):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(one, first))


WIDE_S = 6
WIDE_SEED = 2      # (the third scan step holds 8e-4 of the mass, under one draw in 1000: a seed whose draws reach it in every replicate)
_WIDE = {}


def _wide_definition(mode, bootstrap):
    """(logl, birth, run_start, order, m [WIDE_S, N]) of the definition on _wide(n_runs=24): 528 000 rows, 516 tiles — three
    256-tile steps of the tile scan, the last one of 4 tiles, and the smallest round size past the 1024 blocks at which the
    fixed-point kernel's grid is clamped.  Computed once, shared, never changed."""
    key = (mode, bootstrap)
    if key not in _WIDE:
        if "input" not in _WIDE:
            _WIDE["input"] = _wide(n_runs=24)
        logl, birth, run_start = _WIDE["input"]
        _, _, logwt = merge.replicates_arrays(logl, birth, run_start, WIDE_S, seed=WIDE_SEED, mode=mode, bootstrap=bootstrap,
                                              return_logwt=True)
        out = (merge._layout(logl, birth, run_start)["order"].astype(np.int64), draws.fixed_point(logwt))
        for v in out:
            v.setflags(write=False)
        _WIDE[key] = (logl, birth, run_start) + out
    return _WIDE[key]


@pytest.mark.parametrize("mode, bootstrap", [("random", True), ("expected", False)])
def test_draws_of_516_tiles_land_throughout_the_merged_order_and_are_the_definitions(gpu_required, mode, bootstrap):
    """The first test at 516 tiles, on a fixture whose mass covers the merged order (tests/test_merge_host.py).  The tile scan's
    carry and the parity of its two LDS buffers decide every draw past tile 255: with the definition alone, the 1000 draws of
    every replicate land in at least 400 distinct tiles and in all three 256-tile steps (measured: 470 - 474 tiles), so a scan
    that is wrong from its second step on moves more than half of the draws."""
    logl, birth, run_start, order, m_def = _wide_definition(mode, bootstrap)
    N = logl.size
    assert N == 528_000 and -(-N // 1024) == 516
    seeds = replicate_seeds(WIDE_SEED, WIDE_S)
    for s in range(WIDE_S):
        tiles = np.unique(draws.pick(m_def[s], seeds[s], 1000) // 1024)
        print("replicate", s, "distinct tiles", tiles.size, "steps", sorted(set((tiles // 256).tolist())))
        assert tiles.size >= 400 and set((tiles // 256).tolist()) == {0, 1, 2}
    c_def = np.cumsum(m_def, axis=1, dtype=np.int64)
    bound = 1e-10 * c_def.astype(np.float64) + np.arange(1, N + 1)
    compared = fragile = 0
    for n in (1, 64, 1000):
        rows, logz, info, fixed, msum = draws.device_integers(logl, birth, run_start, n, WIDE_S, seed=WIDE_SEED, mode=mode,
                                                              bootstrap=bootstrap)
        assert np.array_equal(msum, fixed.sum(axis=1, dtype=np.int64)) and fixed.min() >= 0
        assert np.array_equal(rows, _own(order, fixed, seeds, n)), n
        err = np.abs(np.cumsum(fixed, axis=1, dtype=np.int64) - c_def)
        print("n", n, "max |C err| / bound", float((err / bound).max()))
        assert np.all(err <= bound)
        want = _own(order, m_def, seeds, n)
        for s in range(WIDE_S):
            frag = _fragile(c_def[s], seeds[s], n)
            assert np.array_equal(rows[s][~frag], want[s][~frag]), (n, s)
            compared += n
            fragile += int(frag.sum())
    print("fragile draws", fragile, "of", compared)
    assert compared == 6390 and fragile * 1000 <= compared


def test_bits_of_516_tiles_do_not_depend_on_the_batching(gpu_required):
    logl, birth, run_start = _wide_definition("random", True)[:3]
    kw = dict(seed=WIDE_SEED, device=0)
    timing = {}
    one = draws.draw_arrays(logl, birth, run_start, 1000, WIDE_S, timing=timing, **kw)
    assert timing["blocks"] == 1 and timing["tiles"] == 516 and timing["rows"] == logl.size
    few = draws.draw_arrays(logl, birth, run_start, 1000, WIDE_S, block_bytes=8 * logl.size * 2 + 8, timing=timing, **kw)
    assert timing["blocks"] == 3
    assert all(np.array_equal(a, b) for a, b in zip(one, few))
    assert one[0].min() >= 0 and np.unique(one[0][0]).size > 400


@pytest.mark.parametrize("nlive, ndead", [(1, 0), (24, 1000), (25, 1000)])
def test_the_edges_of_the_scans_tile(gpu_required, nlive, ndead):
    rng = np.random.default_rng(nlive)
    logl, birth = _synthetic(rng, nlive, ndead)
    run_start = np.array([0, logl.size], dtype=np.int64)
    assert logl.size in (1, 1024, 1025)
    order = merge._layout(logl, birth, run_start)["order"].astype(np.int64)
    seeds = replicate_seeds(3, 5)
    for n in (1, 7, 300):
        rows, logz, info, fixed, msum = draws.device_integers(logl, birth, run_start, n, 5, seed=3, bootstrap=False)
        assert np.array_equal(rows, _own(order, fixed, seeds, n)) and rows.min() >= 0
        assert np.array_equal(msum, fixed.sum(axis=1, dtype=np.int64))


def test_a_replicate_of_empty_runs_is_minus_one_throughout(gpu_required):
    from test_marginals_host import _with_empty_runs
    logl, birth, run_start, seed = _with_empty_runs()
    rows, logz, _ = draws.draw_arrays(logl, birth, run_start, 5, 12, seed=seed, device=0)
    ref = draws.draw_arrays(logl, birth, run_start, 5, 12, seed=seed)
    dead = np.isneginf(logz)
    assert 0 < dead.sum() < 12 and np.array_equal(dead, np.isneginf(ref[1]))
    assert np.all(rows[dead] == -1) and np.array_equal(rows, ref[0])      # three rows with weights far apart: nothing is fragile


def _raw(ndraws=4, nsamples=2, block_bytes=0, null=(), mode=0, bootstrap=1):
    """rvll_draw_replicates straight from ctypes, past the Python checks, on a fixed four-row merge; returns the code."""
    lib = _abi.load()
    logl, birth = np.array([0.0, 3.0, 1.0, 2.0]), np.array([-np.inf, 0.5, 0.0, -np.inf])
    rs = np.array([0, 2, 4], dtype=np.int64)
    rows = np.zeros((nsamples + 1) * max(1, min(ndraws, 2 ** 20)), np.int32)
    logz, info = np.zeros(nsamples + 1), np.zeros(nsamples + 1)
    return lib.rvll_draw_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), 4, rs.ctypes.data_as(_I64), 2, ndraws, nsamples, mode,
                                    bootstrap, 0, None if "rows" in null else _abi.as_ip(rows),
                                    None if "logz" in null else _abi.as_dp(logz), None if "info" in null else _abi.as_dp(info),
                                    None, None, block_bytes, None)


def test_refusals_by_the_entry_itself(gpu_required):
    assert _raw() == _abi.OK and _raw(ndraws=1) == _abi.OK and _raw(ndraws=2 ** 20, nsamples=1) == _abi.OK
    for bad in (dict(ndraws=0), dict(ndraws=2 ** 20 + 1), dict(ndraws=-1), dict(nsamples=0), dict(mode=2), dict(bootstrap=2),
                dict(block_bytes=-1), dict(null=("rows",)), dict(null=("logz",)), dict(null=("info",))):
        assert _raw(**bad) == _abi.E_INVALID, bad
    assert _raw(block_bytes=31) == _abi.E_NOMEM and _raw(block_bytes=32) == _abi.OK      # one replicate: 8 bytes a row
    logl, birth, run_start = _arrays(_ragged(7))
    with pytest.raises(RvllError) as exc:
        draws.draw_arrays(logl, birth, run_start, 8, 4, device=0, block_bytes=8 * logl.size - 1)
    assert exc.value.code == _abi.E_NOMEM


def test_the_marginal_histograms_keep_their_bits_with_the_shared_fixed_point(gpu_required):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    ref = _reference("random", True)
    kw = dict(nsamples=37, seed=2 ** 64 - 3, mode="random", bootstrap=True, device=0, return_replicates=True)
    dev = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, **kw)
    again = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, **kw)
    _check(dev, ref, 37)
    for key in dev:
        assert np.array_equal(dev[key], again[key], equal_nan=True), key
