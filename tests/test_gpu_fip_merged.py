"""The FIP periodogram of merged runs on the device (rvll_fip_replicates; fip.merged_tip_arrays / merged_fip with device=0) against
the numpy definition of evidence_amd/fip.py: the ragged CPU cases for both shrinkage modes with and without the run bootstrap,
an input of over 2·10^6 rows, a resident 51 Peg ensemble of 16 runs for k = 0 and 1.  The bits are the same from call to call and
in any batching; malformed input is refused by the entry.

Bound.  The merge tests hold every device weight to 1e-12 · max(1, |logwt|) of the definition's, and rows with |logwt| > 50 carry
no mass, so any partial sum of weights is good to 5·10^-11 relative; DELTA = 1e-10 is twice that, as in
test_gpu_posterior.py.  TIP = (A - E) / P is the difference of two such sums, so per bin
    |tip_dev - tip_def| <= 1e-10 (A_def + E_def) / P
and a bin that no row covers is exactly 0 on the device too.  ln Z and H are rvll_merge_replicates' bits.

So that the bound cannot hide a misplaced interval, the synthetic inputs (_local_periods: a row's frequencies rise with its
log-L rank, so a bin collects rows of like weight) are checked with the definition alone: in at least 99 % of the covered
(replicate, bin) pairs the smallest positive row weight that enters the bin is more than 100 times the bound there, so one row
put into or left out of the bin would be seen.  The 51 Peg posterior is what the sampler gave: rows of the prior bulk, with
weights of e^-40 and less, cover every bin, so that margin cannot hold there; its fraction is printed, not asserted.

The 2·10^6-row case stays on _big.  The merge, posterior, marginal and draw tests have a second large input, _wide
(tests/test_gpu_merge.py), whose mass covers the whole merged order, because their bounds are relative to a total that on _big
three rows make up.  The bound here is relative per bin, and _local_periods(by_value=True) spreads rows of every weight over
the grid, so the _big case already weighs rows throughout the merged order.  On _wide with these periods the margin condition
above comes out at 0.9896, under the 0.99 it requires: do not reuse that input here without periods made for it."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, fip, merge, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from evidence_amd.shrinkage import replicate_seeds
from test_gpu_merge import _51peg, _big
from test_merge_host import _arrays, _ragged

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

DELTA = 1e-10


def _local_periods(logl, nplanets, nu, window, seed, by_value=False):
    """Periods [N, nplanets] whose frequencies rise with the row's log-L rank (by_value: with log-L itself, within 4.5 standard
    deviations of its mean) over the inner 90 % of the grid nu, jittered by a window; the other planets sit within a few windows
    of the first: spans that overlap, touch, or stand apart."""
    rng = np.random.default_rng(seed)
    n = logl.size
    rank = np.empty(n)
    rank[np.argsort(logl, kind="stable")] = (np.arange(n) + 0.5) / n
    if by_value:
        rank = np.clip(0.5 + (logl - logl.mean()) / (9.0 * logl.std()), 0.0, 1.0)
    lo, hi = nu[0] + 0.05 * (nu[-1] - nu[0]), nu[-1] - 0.05 * (nu[-1] - nu[0])
    om = (lo + (hi - lo) * rank + window * rng.uniform(-1.0, 1.0, n))[:, None]
    shift = window * rng.choice([0.0, 0.3, 1.0, 1.7, 3.0], (n, nplanets)) * rng.choice([-1.0, 1.0], (n, nplanets))
    shift[:, 0] = 0.0
    return 2 * np.pi / np.maximum(om + shift, 0.5 * nu[0])


def _min_entering_weight(beg, end, p, nfreq):
    """Per bin the smallest positive p of a row that covers it (inf where there is none)."""
    out = np.full(nfreq, np.inf)
    for k in range(beg.shape[1]):
        rows = np.flatnonzero((beg[:, k] < nfreq) & (p > 0.0))
        length = end[rows, k] - beg[rows, k]
        start = np.cumsum(length) - length
        bins = np.repeat(beg[rows, k], length) + (np.arange(length.sum()) - np.repeat(start, length))
        np.minimum.at(out, bins, np.repeat(p[rows], length))
    return out


def _reference(periods, logl, birth, run_start, nua, nub, nrep, seed=0, mode="random", bootstrap=True):
    """The definition's first nrep replicates with A / P and E / P, and the fraction of covered (replicate, bin) pairs in which
    the smallest entering weight is more than 100 times the bound."""
    logl, birth, run_start, _, code = merge.check_args(logl, birth, run_start, nrep, mode, bootstrap)
    periods, nua, nub = fip.check_merged_args(periods, logl, nua, nub)
    prep = fip._prepare(periods, logl, birth, run_start, nua, nub)
    logz, info, tip, a, e = fip._definition_block(prep, replicate_seeds(seed, nrep), code == _abi.SHRINK_EXPECTED, bootstrap,
                                                  parts=True)
    beg, end = fip.row_intervals(periods[prep["lay"]["order"]], nua, nub)
    covered = prep["cnt_a"] != prep["cnt_e"]
    logwt = merge.replicates_arrays(logl, birth, run_start, nrep, seed, mode, bootstrap, return_logwt=True)[2]
    clear = total = 0
    for s in range(nrep):
        p = np.exp(logwt[s])
        low = _min_entering_weight(beg, end, p / p.sum(), nua.size)
        clear += int((low[covered] > 100 * DELTA * (a[s] + e[s])[covered]).sum())
        total += int(covered.sum())
    return dict(logz=logz, information=info, tip=tip, a=a, e=e, covered=covered, clear=clear / max(total, 1))


def _check(dev, ref, nrep):
    """The first nrep replicates of the device result against the definition's."""
    got, want, slack = dev["tip"][:nrep], ref["tip"][:nrep], DELTA * (ref["a"] + ref["e"])[:nrep]
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(slack > 0, err / slack, np.where(err > 0, np.inf, 0.0))))
    print("max |tip err| / (1e-10 (A + E) / P):", worst, " equal bins:", int((got == want).sum()), "of", got.size,
          " covered bins:", int(ref["covered"].sum()), " margin fraction:", ref["clear"])
    assert np.all(err <= slack), worst
    assert np.all(got[:, ~ref["covered"]] == 0.0) and not np.signbit(got[:, ~ref["covered"]]).any()
    assert np.all((got >= 0.0) & (got <= 1.0))


def _ragged_case(nplanets, nfreq=400):
    logl, birth, run_start = _arrays(_ragged(5))
    nu, nua, nub = fip.frequency_grid(1.5, 200.0, 300.0, nfreq=nfreq)
    return logl, birth, run_start, _local_periods(logl, nplanets, nu, nub[0] - nua[0], 3 + nplanets), nua, nub


@pytest.mark.parametrize("nplanets", [1, 3])
@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_tip_matches_the_definition(gpu_required, mode, bootstrap, nplanets):
    logl, birth, run_start, periods, nua, nub = _ragged_case(nplanets)
    kw = dict(seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap)
    ref = _reference(periods, logl, birth, run_start, nua, nub, 37, **kw)
    assert ref["clear"] >= 0.99 and (~ref["covered"]).sum() > 0 and ref["covered"].sum() > 100
    timing = {}
    dev = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=37, device=0, timing=timing, **kw)
    _check(dev, ref, 37)
    plain = merge.replicates_arrays(logl, birth, run_start, 37, device=0, **kw)
    assert np.array_equal(plain[0], dev["logz"]) and np.array_equal(plain[1], dev["information"])
    assert timing["rows"] == logl.size and timing["elements"] == 37 * logl.size and timing["blocks"] == 1
    assert timing["events"] == 2 * logl.size * nplanets and timing["key_bits"] == 9
    assert timing["launches"] == 11 + 4 and timing["kernel_ms"] > 0


def test_peaked_and_out_of_grid_periods(gpu_required):
    """Every row in one window (one bin's read position many tiles into the list), rows off both ends of the grid, and rows
    with eight planets of which some repeat."""
    logl, birth, run_start = _arrays(_ragged(6) + _ragged(7) + _ragged(8))
    n = logl.size
    nu, nua, nub = fip.frequency_grid(1.5, 200.0, 300.0, nfreq=700)
    rng = np.random.default_rng(2)
    peak = np.full((n, 1), 4.2307) * (1.0 + 1e-7 * rng.normal(size=(n, 1)))
    dev = fip.merged_tip_arrays(peak, logl, birth, run_start, nua, nub, nsamples=5, seed=1, device=0)
    ref = _reference(peak, logl, birth, run_start, nua, nub, 5, seed=1)
    _check(dev, ref, 5)
    assert n > 1024 and np.all(np.abs(dev["tip"].max(axis=1) - 1.0) <= 1e-12)
    wide = np.exp(rng.uniform(np.log(0.3), np.log(3000.0), (n, 8)))
    wide[:, 5] = wide[:, 2]
    dev = fip.merged_tip_arrays(wide, logl, birth, run_start, nua, nub, nsamples=5, seed=1, device=0)
    _check(dev, _reference(wide, logl, birth, run_start, nua, nub, 5, seed=1), 5)
    off = np.concatenate([np.full((n // 2, 1), 0.5), np.full((n - n // 2, 1), 5000.0)])
    dev = fip.merged_tip_arrays(off, logl, birth, run_start, nua, nub, nsamples=3, seed=1, device=0)
    assert np.all(dev["tip"] == 0.0)


def test_bits_are_stable_in_any_batching_and_from_call_to_call(gpu_required):
    logl, birth, run_start, periods, nua, nub = _ragged_case(3)
    kw = dict(nsamples=9, seed=11, device=0)
    one = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, **kw)
    again = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, **kw)
    timing = {}
    small = fip.merged_table_bytes(logl.size, 3, nua.size) + 2 * (8 * logl.size + 16 * nua.size) + 8
    few = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, timing=timing, block_bytes=small, **kw)
    assert timing["blocks"] == 5 and timing["launches"] == 11 + 4 * 5
    first = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=1, seed=11, device=0)
    for key in one:
        assert np.array_equal(one[key], again[key]), key
        assert np.array_equal(one[key], few[key]), key
        assert np.array_equal(one[key][0], first[key][0]), key
    # replicates s0 .. of a call are the call with the seed moved on by s0 replicates
    from evidence_amd.shrinkage import SEED_MUL
    tail = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=4, seed=(11 + 5 * SEED_MUL) % 2 ** 64, device=0)
    assert np.array_equal(tail["tip"], one["tip"][5:])


def test_two_million_rows_match_the_definition_on_the_first_replicates(gpu_required):
    logl, birth, run_start = _big()
    n = logl.size
    assert n > 2_000_000
    nu, nua, nub = fip.frequency_grid(1.5, 1000.0, 40000.0, nfreq=fip.NFREQ)       # windows of about two bins
    periods = _local_periods(logl, 2, nu, nub[0] - nua[0], 1, by_value=True)
    # The margin is asserted for the expected shrinkage.  With random shrinkage a weight carries its own -log u ~ Exp(1), a bin here
    # is entered by some 10^3 rows and A + E sum some 4·10^4 like weights, so the smallest entering weight falls below
    # 100 x 1e-10 (A + E) in a few per cent of the bins whatever the periods: those replicates are held to the bound alone.
    kw = dict(seed=3, mode="expected", bootstrap=True)
    ref = _reference(periods, logl, birth, run_start, nua, nub, 2, **kw)
    assert ref["clear"] >= 0.99
    timing = {}
    dev = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=24, device=0, timing=timing, **kw)
    print("timing", timing)
    assert timing["elements"] == 24 * n and timing["rows"] == n and timing["events"] == 4 * n and timing["key_bits"] == 16
    _check(dev, ref, 2)
    assert np.all(np.isfinite(dev["tip"])) and np.all((dev["tip"] >= 0) & (dev["tip"] <= 1))
    assert np.all(dev["tip"][:, ~ref["covered"]] == 0.0)
    kw = dict(seed=3, mode="random", bootstrap=True)
    dev = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=8, device=0, **kw)
    _check(dev, _reference(periods, logl, birth, run_start, nua, nub, 2, **kw), 2)


def _raw(periods=None, n_planets=None, nua=(0.0, 1.0, 2.0), nub=(1.0, 2.0, 3.0), nfreq=None, block_bytes=0, null=None, nsamples=2,
         mode=0, bootstrap=1):
    """rvll_fip_replicates straight from ctypes, past the Python checks, on a fixed four-row merge; returns the code."""
    lib = _abi.load()
    logl, birth = np.array([0.0, 3.0, 1.0, 2.0]), np.array([-np.inf, 0.5, 0.0, -np.inf])
    rs = np.array([0, 2, 4], dtype=np.int64)
    periods = np.ascontiguousarray(GOOD if periods is None else periods, dtype=np.float64)
    nua, nub = np.ascontiguousarray(nua, dtype=np.float64), np.ascontiguousarray(nub, dtype=np.float64)
    n_planets = periods.size // 4 if n_planets is None else n_planets
    nfreq = nua.size if nfreq is None else nfreq
    out = {k: np.zeros(max(nsamples, 1) * max(nfreq, 1) + 1) for k in ("logz", "info", "tip")}
    ptr = {k: _abi.as_dp(v) for k, v in out.items()}
    ptr.update(periods=_abi.as_dp(periods), nua=_abi.as_dp(nua), nub=_abi.as_dp(nub))
    if null:
        ptr[null] = None
    return lib.rvll_fip_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), 4, rs.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                   ptr["periods"], n_planets, ptr["nua"], ptr["nub"], nfreq, nsamples, mode, bootstrap, 0,
                                   ptr["logz"], ptr["info"], ptr["tip"], block_bytes, None)


GOOD = [[4.0, 9.0], [3.0, 2.5], [5.0, 6.0], [7.0, 8.0]]


@pytest.mark.parametrize("args", [
    dict(null="periods"), dict(null="nua"), dict(null="nub"), dict(null="logz"), dict(null="info"), dict(null="tip"),
    dict(n_planets=0),
    dict(periods=np.ones((4, 9))),
    dict(nfreq=0),
    dict(nub=(1.0, 3.0, 2.0)),
    dict(nua=(0.0, 2.0, 1.0)),
    dict(nub=(1.0, np.nan, 3.0)),
    dict(periods=[[4.0, 9.0], [np.nan, 2.5], [5.0, 6.0], [7.0, 8.0]]),
    dict(periods=[[4.0, 9.0], [3.0, 2.5], [5.0, np.inf], [7.0, 8.0]]),
    dict(periods=[[4.0, 9.0], [3.0, 2.5], [5.0, 6.0], [0.0, 8.0]]),
    dict(periods=[[4.0, -9.0], [3.0, 2.5], [5.0, 6.0], [7.0, 8.0]]),
    dict(mode=2),
    dict(bootstrap=2),
    dict(nsamples=0),
    dict(block_bytes=-1),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    assert _raw(**args) == _abi.E_INVALID
    assert _raw() == _abi.OK
    assert _raw(np.ones((4, 8))) == _abi.OK


def test_what_merge_refuses_is_refused(gpu_required):
    logl, birth, run_start, periods, nua, nub = _ragged_case(1)
    lib = _abi.load()

    def call(logl=logl, birth=birth, rs=run_start):
        out = [np.zeros(2 * nua.size) for _ in range(3)]
        return lib.rvll_fip_replicates(0, _abi.as_dp(np.ascontiguousarray(logl)), _abi.as_dp(np.ascontiguousarray(birth)),
                                       len(logl), np.ascontiguousarray(rs).ctypes.data_as(C.POINTER(C.c_int64)), len(rs) - 1,
                                       _abi.as_dp(periods), 1, _abi.as_dp(nua), _abi.as_dp(nub), nua.size, 2, 0, 1, 0,
                                       *[_abi.as_dp(o) for o in out], 0, None)

    bad_l, bad_b = logl.copy(), birth.copy()
    bad_l[3], bad_b[0] = np.nan, np.nan
    assert call() == _abi.OK
    assert call(logl=bad_l) == _abi.E_INVALID and call(birth=bad_b) == _abi.E_INVALID
    assert call(rs=np.r_[run_start[:-1], run_start[-1] - 1]) == _abi.E_INVALID


def test_a_block_bound_one_byte_short_is_refused_with_nomem(gpu_required):
    logl, birth, run_start, periods, nua, nub = _ragged_case(3)
    need = fip.merged_table_bytes(logl.size, 3, nua.size) + 8 * logl.size + 16 * nua.size
    with pytest.raises(RvllError) as exc:
        fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=4, device=0, block_bytes=need - 1)
    assert exc.value.code == _abi.E_NOMEM
    timing = {}
    exact = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=4, device=0, block_bytes=need, timing=timing)
    assert timing["blocks"] == 4
    roomy = fip.merged_tip_arrays(periods, logl, birth, run_start, nua, nub, nsamples=4, device=0)
    assert all(np.array_equal(exact[k], roomy[k]) for k in exact)
    small = fip.merged_table_bytes(4, 2, 3) + 8 * 4 + 16 * 3
    assert _raw(block_bytes=small - 1) == _abi.E_NOMEM and _raw(block_bytes=small) == _abi.OK


def _51peg_null():
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=0)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict), datadict


def test_51peg_merged_fip_from_resident_ensembles(gpu_required):
    seeds = list(range(1, 17))
    null, datadict = _51peg_null()
    with null as m:
        r0 = run_nested_ensemble(None, None, m.ndim, seeds, live=m, nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames),
                                 max_calls=16_000_000)
    with _51peg() as m:
        col = m.parnames.index("planet1_period")
        r1 = run_nested_ensemble(None, None, m.ndim, seeds, live=m, nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames),
                                 max_calls=16_000_000)
    nu, nua, nub = fip.frequency_grid(1.5, 1000.0, fip.observation_span(datadict))
    timing = {}
    dev = fip.merged_fip([r0, r1], [[], [col]], nua, nub, nsamples=200, seed=7, device=0, nu=nu, return_replicates=True,
                         timing=timing)
    best = int(np.argmin(dev["log10fip"]))
    print(f"lowest log10 FIP {dev['log10fip'][best]:.3f} +/- {dev['log10fip_err'][best]:.3f} at P = {dev['periods'][best]:.4f} d; "
          f"p(k | y) = {dev['pky']} +/- {dev['pky_err']}; ln Z = {dev['logz']} +/- {dev['logz_err']}; timing {timing}")
    w = 2 * np.pi / 4.2307
    assert nua[best] - (nub[0] - nua[0]) <= w <= nub[best] + (nub[0] - nua[0])          # within one window of 51 Peg b
    for key in ("log10fip_err", "pky_err", "logz_err", "log10fip_min", "log10fip_max", "fip", "log10fip"):
        assert np.all(np.isfinite(dev[key])), key
    assert np.all(dev["log10fip_min"] <= dev["log10fip_max"])
    assert dev["logz_err"].min() > 0 and dev["log10fip_err"][best] >= 0
    # the k = 1 model alone against the definition, replicate by replicate
    _, logl, birth, run_start = merge._stack(r1)
    per = np.concatenate([np.asarray(r.samples)[:, [col]] for r in r1])
    kw = dict(seed=fip.model_seed(7, 1), mode="random", bootstrap=True)
    tip = fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=3, device=0, **kw)
    ref = _reference(per, logl, birth, run_start, nua, nub, 3, **kw)
    _check(tip, ref, 3)
    # and the combination on the first replicates: ln Z is good to 1e-12 |ln Z| (the merge tests), so ln p(k | y), a difference
    # of two of them, to twice that, and 1 - FIP = p(1 | y) * tip to that relative error next to the bound of tip
    host = fip.merged_fip([r0, r1], [[], [col]], nua, nub, nsamples=3, seed=7, return_replicates=True)
    top = np.abs(host["logz_replicates"]).max()
    assert np.max(np.abs(host["logz_replicates"] - dev["logz_replicates"][:3])) <= 1e-12 * top
    slack = DELTA * (ref["a"] + ref["e"]) + 2e-12 * top * np.abs(1.0 - host["replicates"]) + 4 * np.finfo(float).eps
    assert np.all(np.abs(host["replicates"] - dev["replicates"][:3]) <= slack)
