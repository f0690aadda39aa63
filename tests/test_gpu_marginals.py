"""Marginal histograms on the device (rvll_marginal_replicates; marginals.marginals_arrays / marginals with device=0) against the
numpy definition of evidence_amd/marginals.py: 3212 ragged rows (four row chunks, two panel groups) for both shrinkage modes with
and without the run bootstrap, degenerate panels, a replicate of empty runs, an input of over 2·10^6 rows, a resident 51 Peg
ensemble of 16 runs.  The bits are the same from call to call, in any batching, for a panel alone and in any order of the panels;
malformed input is refused by the entry.

Bounds.  counts and outside_count are integers and must equal the definition's exactly, which pins the binning whatever the
weights.  The merge tests hold every device weight to 1e-12 · max(1, |logwt|) of the definition's, and rows with |logwt| > 50
carry no mass, so any partial sum of weights is good to 5·10^-11 relative; 1e-10 is twice that.  Each of the n_b rows of a bin is
rounded to a multiple of 2^-62 on either side, and so is the total: with mass_def the definition's mass of the bin

    |mass_dev - mass_def| <= 1e-10 mass_def + (n_b + 1) 2^-61

and a bin without rows has mass exactly 0.  The same holds for the mass outside a panel.  mean, min and max over the replicates
are held to the largest such bound of the bin, the standard deviation to twice that."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import RvllError, _abi, marginals, merge, run_nested_ensemble
from evidence_amd.callbacks import wrapped_params
from test_gpu_merge import _51peg, _big, _close, _wide
from test_marginals_host import _case, _small, _with_empty_runs
from test_merge_host import _arrays, _ragged
from test_posterior_host import _columns

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

_I64 = C.POINTER(C.c_int64)
_REFS = {}


def _reference(mode, bootstrap):
    """The definition on the small input, S = 37, seed 2^64 - 3: computed once, shared, never changed."""
    key = (mode, bootstrap)
    if key not in _REFS:
        logl, birth, run_start = _small()
        values, axes, panels = _case(logl.size)
        ref = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=37, seed=2 ** 64 - 3, mode=mode,
                                         bootstrap=bootstrap, return_replicates=True)
        for v in ref.values():
            v.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


def _bounds(ref, nrep):
    """Per (replicate, bin) and per (replicate, panel) the bound of the module's docstring."""
    bins = 1e-10 * ref["mass"][:nrep] + (ref["counts"] + 1) * 2.0 ** -61
    out = 1e-10 * ref["outside"][:nrep] + (ref["outside_count"] + 1) * 2.0 ** -61
    return bins, out


def _check(dev, ref, nrep, stats=True):
    assert dev["counts"].dtype == np.int64 and np.array_equal(dev["counts"], ref["counts"])
    assert np.array_equal(dev["outside_count"], ref["outside_count"]) and np.array_equal(dev["panel_start"], ref["panel_start"])
    bins, out = _bounds(ref, nrep)
    err, oerr = np.abs(dev["mass"][:nrep] - ref["mass"][:nrep]), np.abs(dev["outside"][:nrep] - ref["outside"][:nrep])
    print("max |mass err| / bound", float((err / bins).max()), " max |outside err| / bound", float((oerr / out).max()),
          " bins with mass", int((ref["mass"][:nrep] > 0).sum()), "of", err.size)
    assert np.all(err <= bins), float((err / bins).max())
    assert np.all(oerr <= out), float((oerr / out).max())
    assert np.all(dev["mass"][:, ref["counts"] == 0] == 0.0) and np.all(dev["outside"][:, ref["outside_count"] == 0] == 0.0)
    if stats:
        top = bins.max(axis=0)
        for key, k in (("mean", 1), ("min", 1), ("max", 1), ("std", 2)):
            e = np.abs(dev[key] - ref[key])
            print(key, "max err / bound", float((e / (k * top)).max()))
            assert np.all(e <= k * top), key


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_histograms_match_the_definition(gpu_required, mode, bootstrap):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    ref = _reference(mode, bootstrap)
    kw = dict(seed=2 ** 64 - 3, mode=mode, bootstrap=bootstrap)
    timing = {}
    dev = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=37, device=0, return_replicates=True,
                                     timing=timing, **kw)
    _check(dev, ref, 37)
    plain = merge.replicates_arrays(logl, birth, run_start, 37, device=0, **kw)
    assert np.array_equal(plain[0], dev["logz"]) and np.array_equal(plain[1], dev["information"])
    _close(dev["logz"], ref["logz"])
    print("timing", timing)
    assert timing["rows"] == logl.size and timing["elements"] == 37 * logl.size and timing["bins"] == ref["counts"].size
    assert timing["blocks"] == 1 and timing["launches"] == 6 + 4 and timing["groups"] == 2 and timing["kernel_ms"] > 0


def test_bits_are_stable_in_any_batching_grouping_and_from_call_to_call(gpu_required):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    kw = dict(nsamples=9, seed=11, device=0, return_replicates=True)
    one = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, **kw)
    again = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, **kw)
    timing = {}
    nbins = int(one["panel_start"][-1])
    few = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, timing=timing, block_bytes=marginals.table_bytes(
        logl.size, len(axes)) + 2 * marginals.replicate_bytes(logl.size, nbins, len(panels)) + 8, **kw)
    assert timing["blocks"] == 5 and timing["launches"] == 6 + 4 * 5
    first = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, **dict(kw, nsamples=1))
    for key in one:
        assert np.array_equal(one[key], again[key]), key
        assert np.array_equal(one[key], few[key]), key                  # the statistics too: the Welford state crosses blocks
    for key in ("mass", "outside", "logz", "information"):
        assert np.array_equal(one[key][0], first[key][0]), key
    assert np.array_equal(first["mean"], first["mass"][0]) and np.all(first["std"] == 0.0)
    start = one["panel_start"]
    for t in (5, 7, 10):                                                 # a panel alone: 4096 bins, 40 x 40, 64 x 64
        pan = panels[t]
        ax, p = ([axes[pan]], [0]) if isinstance(pan, int) else ([axes[pan[0]], axes[pan[1]]], [(0, 1)])
        alone = marginals.marginals_arrays(values, logl, birth, run_start, ax, p, **kw)
        sl = slice(int(start[t]), int(start[t + 1]))
        for key in ("counts", "mean", "std", "min", "max"):
            assert np.array_equal(alone[key], one[key][sl]), (t, key)
        assert np.array_equal(alone["mass"], one["mass"][:, sl]) and np.array_equal(alone["outside"][:, 0], one["outside"][:, t])
        assert alone["outside_count"][0] == one["outside_count"][t]
    back = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels[::-1], **kw)   # other groups, other offsets
    bstart = back["panel_start"]
    for t in range(len(panels)):
        u = len(panels) - 1 - t
        sl, bl = slice(int(start[t]), int(start[t + 1])), slice(int(bstart[u]), int(bstart[u + 1]))
        for key in ("counts", "mean", "std", "min", "max"):
            assert np.array_equal(back[key][bl], one[key][sl]), (t, key)
        assert np.array_equal(back["mass"][:, bl], one["mass"][:, sl]) and np.array_equal(back["outside"][:, u], one["outside"][:, t])


def test_degenerate_panels(gpu_required):
    logl, birth, run_start = _small()
    values, axes, panels = _case(logl.size)
    dev = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=12, seed=1, device=0,
                                     return_replicates=True)
    start = dev["panel_start"]
    const = dev["mass"][:, start[3]:start[4]]                            # the constant column: edges 1234, 1234.5678, 1235, 1300
    assert dev["outside_count"][3] == 0 and np.all(dev["outside"][:, 3] == 0.0)
    assert np.all(const[:, 1] == 1.0) and np.all(const[:, 0] == 0.0) and np.all(const[:, 2] == 0.0)
    assert list(dev["counts"][start[3]:start[4]]) == [0, logl.size, 0]
    # a panel of one bin: h / M and (M - h) / M, each rounded once, a subtraction rounded once: 2^-52 covers the three
    one = dev["mass"][:, start[6]]
    assert dev["outside_count"][6] > 0 and np.all(np.abs(one - (1.0 - dev["outside"][:, 6])) <= 2.0 ** -52)
    assert np.all((one > 0) & (one < 1))
    assert np.all(dev["min"] <= dev["mean"] + 2.0 ** -52) and np.all(dev["mean"] <= dev["max"] + 2.0 ** -52)
    assert np.all(dev["std"] >= 0)


def test_a_replicate_of_empty_runs_is_nan_and_skipped(gpu_required):
    logl, birth, run_start, seed = _with_empty_runs()
    args = (np.arange(3.0), logl, birth, run_start, [(0, [-1.0, 0.5, 3.0])], [0])
    ref = marginals.marginals_arrays(*args, nsamples=12, seed=seed, return_replicates=True)
    dev = marginals.marginals_arrays(*args, nsamples=12, seed=seed, return_replicates=True, device=0)
    dead = np.isnan(ref["mass"][:, 0])
    assert 0 < dead.sum() < 12
    assert np.array_equal(np.isnan(dev["mass"]), np.isnan(ref["mass"])) and np.array_equal(np.isnan(dev["outside"]),
                                                                                            np.isnan(ref["outside"]))
    assert np.array_equal(np.isneginf(dev["logz"]), dead)
    live = {k: (v[~dead] if k in ("mass", "outside") else v) for k, v in dev.items()}
    want = {k: (v[~dead] if k in ("mass", "outside") else v) for k, v in ref.items()}
    _check(live, want, int((~dead).sum()))
    assert np.all(np.isfinite(dev["mean"])) and np.all(np.isfinite(dev["std"]))
    one = marginals.marginals_arrays(*args, nsamples=int(np.flatnonzero(dead)[0]) + 1, seed=seed, device=0)
    if np.flatnonzero(dead)[0] == 0:                                     # nothing but a dead replicate: no statistics
        assert np.all(np.isnan(one["mean"])) and np.all(np.isnan(one["std"]))


def test_two_million_rows_match_the_definition_on_the_first_replicates(gpu_required):
    logl, birth, run_start = _big()
    n = logl.size
    assert n > 2_000_000
    rng = np.random.default_rng(1)
    values = np.stack([rng.normal(0.0, 3.0, n), np.round(rng.normal(2.0, 0.5, n), 1), 4.23 + 1e-5 * rng.normal(size=n),
                       np.exp(rng.uniform(0.0, 7.0, n)), 0.01 * (logl + 500.0) + rng.normal(0.0, 0.1, n),
                       rng.integers(0, 5, n).astype(float)], axis=1)
    lo, hi = values.min(axis=0), values.max(axis=0)
    span = hi - lo
    axes = [(c, np.linspace(lo[c] + 0.02 * span[c], hi[c] - 0.02 * span[c], 201)) for c in range(6)]
    axes += [(c, np.linspace(lo[c], hi[c], 41)) for c in range(6)]
    panels = list(range(6)) + [(6 + a, 6 + b) for a in range(6) for b in range(a + 1, 6)]
    assert len(panels) == 21
    kw = dict(seed=3, mode="random", bootstrap=True)
    timing = {}
    dev = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=16, device=0, return_replicates=True,
                                     timing=timing, **kw)
    print("timing", timing)
    assert timing["elements"] == 16 * n and timing["rows"] == n and timing["bins"] == 6 * 200 + 15 * 1600
    ref = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=2, return_replicates=True, **kw)
    _check(dev, ref, 2, stats=False)
    assert dev["outside_count"][:6].min() > 0 and np.all(dev["outside_count"][6:] == 0)
    assert all(np.all(np.isfinite(v)) for v in dev.values()) and np.all(dev["mass"] >= 0) and np.all(dev["outside"] >= 0)
    start = dev["panel_start"]
    total = np.add.reduceat(dev["mass"], start[:-1], axis=1) + dev["outside"]
    assert np.all(np.abs(total - 1.0) <= 1e-9), float(np.abs(total - 1.0).max())
    assert np.all(dev["min"] <= dev["max"]) and np.all(dev["std"] >= 0)


def _wide_case():
    """_wide with the posterior tests' six columns (column 4 follows log-L) and the axes and panels of the test above."""
    logl, birth, run_start = _wide()
    n = logl.size
    rng = np.random.default_rng(1)
    values = np.stack([rng.normal(0.0, 3.0, n), np.round(rng.normal(2.0, 0.5, n), 1), 4.23 + 1e-5 * rng.normal(size=n),
                       np.exp(rng.uniform(0.0, 7.0, n)), logl + rng.normal(0.0, 0.1, n),
                       rng.integers(0, 5, n).astype(float)], axis=1)
    lo, hi = values.min(axis=0), values.max(axis=0)
    span = hi - lo
    axes = [(c, np.linspace(lo[c] + 0.02 * span[c], hi[c] - 0.02 * span[c], 201)) for c in range(6)]
    axes += [(c, np.linspace(lo[c], hi[c], 41)) for c in range(6)]
    panels = list(range(6)) + [(6 + a, 6 + b) for a in range(6) for b in range(a + 1, 6)]
    return values, logl, birth, run_start, axes, panels


def test_two_million_rows_of_spread_mass_match_the_definition(gpu_required):
    """The histograms of _wide, whose mass covers the merged order (tests/test_merge_host.py): every bin's mass is a sum over
    rows of every tile, 8e-4 of it from rows past 2^21 (the second grid-stride pass), so a bin kernel or a replicate carry that
    loses rows is outside the bound here where on _big it would lose nothing that has weight.

    The case has not degenerated: in the definition, more than half of the bins of every 1-D panel hold mass.  A bin holds
    mass only if a value of its column falls into it, and columns 1 and 5 take 48 and 3 values inside their 200 bins, so the
    count is held against min(bins, distinct values inside the panel): the bins themselves for the other four columns."""
    values, logl, birth, run_start, axes, panels = _wide_case()
    n = logl.size
    assert n > 2 ** 21 + 8192 and len(panels) == 21
    kw = dict(seed=3, mode="random", bootstrap=True)
    timing = {}
    dev = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=4, device=0, return_replicates=True,
                                     timing=timing, **kw)
    print("timing", timing)
    assert timing["elements"] == 4 * n and timing["rows"] == n and timing["bins"] == 6 * 200 + 15 * 1600
    ref = marginals.marginals_arrays(values, logl, birth, run_start, axes, panels, nsamples=2, return_replicates=True, **kw)
    start = ref["panel_start"]
    for c in range(6):
        edges = axes[c][1]
        col = values[:, c]
        attainable = min(200, np.unique(col[(col >= edges[0]) & (col < edges[-1])]).size)
        held = (ref["mass"][:, start[c]:start[c + 1]] > 0).sum(axis=1)
        print("panel", c, "bins with mass", held, "attainable", attainable)
        assert np.all(held > 0.5 * attainable), (c, held, attainable)
    _check(dev, ref, 2, stats=False)
    assert dev["outside_count"][:6].min() > 0 and np.all(dev["outside_count"][6:] == 0)
    assert all(np.all(np.isfinite(v)) for v in dev.values()) and np.all(dev["mass"] >= 0) and np.all(dev["outside"] >= 0)
    total = np.add.reduceat(dev["mass"], start[:-1], axis=1) + dev["outside"]
    print("max |mass + outside - 1|", float(np.abs(total - 1.0).max()))
    assert np.all(np.abs(total - 1.0) <= 1e-9), float(np.abs(total - 1.0).max())
    assert np.all(dev["min"] <= dev["max"]) and np.all(dev["std"] >= 0)


def test_51peg_period_marginal_from_a_resident_ensemble(gpu_required):
    with _51peg() as m:
        names = list(m.parnames)
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, 17)), live=m, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=16_000_000)
    timing = {}
    dev = marginals.marginals(got, names, nsamples=200, seed=7, device=0, timing=timing)
    print("timing", timing)
    ncol = len(names)
    assert len(dev["panels"]) == ncol + ncol * (ncol - 1) // 2
    period = dev["panels"][names.index("planet1_period")]
    assert period["columns"] == ("planet1_period",)
    top = int(np.argmax(period["density"]))
    edges = period["edges"][0]
    print("period bin", edges[top], edges[top + 1], "density", period["density"][top], "+/-", period["density_err"][top],
          "in", period["density_min"][top], period["density_max"][top])
    # 51 Peg b's period is 4.2307 d to the digits given.  The 40 bins over the [1e-4, 1 - 1e-4] quantile range are 8e-6 d wide
    # (the mode bin measured here: [4.2307231, 4.2307309], the posterior mean being 4.230729), so the point 4.2307000 itself is
    # four bins below the mode; the whole mode bin must lie among the numbers that are written 4.2307
    assert 4.23065 <= edges[top] and edges[top + 1] <= 4.23075
    assert period["density_err"][top] > 0 and period["density_min"][top] <= period["density_max"][top]
    _, cols, logl, birth, run_start = marginals.posterior._values(got, None, None, False, names)
    point = marginals.marginals_arrays(cols, logl, birth, run_start, [(names.index("planet1_period"), edges)], [0], nsamples=1,
                                       mode="expected", bootstrap=False, device=0, return_replicates=True)
    assert np.array_equal(point["mass"][0] / np.diff(edges), period["density"])
    assert np.array_equal(point["counts"], period["counts"])
    ref = marginals.marginals_arrays(cols, logl, birth, run_start, [(names.index("planet1_period"), edges)], [0], nsamples=1,
                                     mode="expected", bootstrap=False, return_replicates=True)
    _check(point, ref, 1)
    pair = dev["panels"][ncol]
    lv = marginals.credible_levels(pair["mass"])
    assert pair["mass"].shape == (40, 40) and lv[0] >= lv[1] > 0


def _raw(values=None, edges=(0.0, 4.0, 9.0), axis_col=(0,), axis_start=(0, 3), panel_axes=((0, -1),), n_cols=None, n_axes=None,
         n_panels=None, block_bytes=0, null=(), nsamples=2, mode=0, bootstrap=1):
    """rvll_marginal_replicates straight from ctypes, past the Python checks, on a fixed four-row merge; returns the code."""
    lib = _abi.load()
    logl, birth = np.array([0.0, 3.0, 1.0, 2.0]), np.array([-np.inf, 0.5, 0.0, -np.inf])
    rs = np.array([0, 2, 4], dtype=np.int64)
    values = np.ascontiguousarray(GOOD if values is None else values, dtype=np.float64)
    a = dict(values=values, edges=np.ascontiguousarray(edges, dtype=np.float64), axis_col=np.ascontiguousarray(axis_col, dtype=np.int32),
             axis_start=np.ascontiguousarray(axis_start, dtype=np.int64),
             panel_axes=np.ascontiguousarray(panel_axes, dtype=np.int32).reshape(-1))
    n_cols = values.size // 4 if n_cols is None else n_cols
    n_axes = a["axis_col"].size if n_axes is None else n_axes
    n_panels = a["panel_axes"].size // 2 if n_panels is None else n_panels
    a.update(logz=np.zeros(nsamples + 1), info=np.zeros(nsamples + 1), counts=np.zeros(16384, np.int64),
             outside_count=np.zeros(512, np.int64), stats=np.zeros(4 * 16384), mass=np.zeros((nsamples + 1) * 16384),
             outside=np.zeros((nsamples + 1) * 512))
    ptr = {}
    for k, v in a.items():
        if k in null:
            ptr[k] = None
        elif v.dtype == np.int64:
            ptr[k] = v.ctypes.data_as(_I64)
        elif v.dtype == np.int32:
            ptr[k] = _abi.as_ip(v)
        else:
            ptr[k] = _abi.as_dp(v)
    return lib.rvll_marginal_replicates(0, _abi.as_dp(logl), _abi.as_dp(birth), 4, rs.ctypes.data_as(_I64), 2, ptr["values"], n_cols,
                                        ptr["edges"], ptr["axis_col"], ptr["axis_start"], n_axes, ptr["panel_axes"], n_panels,
                                        nsamples, mode, bootstrap, 0, ptr["logz"], ptr["info"], ptr["counts"],
                                        ptr["outside_count"], ptr["stats"], ptr["mass"], ptr["outside"], block_bytes, None)


GOOD = [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0]]


@pytest.mark.parametrize("args", [
    dict(values=[[1.0, 2.0], [np.nan, 4.0], [5.0, 6.0], [7.0, 8.0]]),
    dict(values=[[1.0, 2.0], [3.0, 4.0], [5.0, np.inf], [7.0, 8.0]]),
    dict(values=[[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [-np.inf, 8.0]]),
    dict(n_cols=0),
    dict(values=np.zeros((4, 65))),
    dict(n_axes=0),
    dict(edges=np.arange(258.0), axis_col=[0] * 129, axis_start=np.arange(0, 259, 2)),
    dict(n_panels=0),
    dict(panel_axes=[(0, -1)] * 257),
    dict(edges=[0.0], axis_start=(0, 1)),
    dict(edges=np.arange(4098.0), axis_start=(0, 4098)),
    dict(edges=[0.0, 4.0, 4.0]),
    dict(edges=[0.0, 4.0, 3.0]),
    dict(edges=[0.0, np.nan, 9.0]),
    dict(edges=[0.0, 4.0, np.inf]),
    dict(edges=[-np.inf, 4.0, 9.0]),
    dict(axis_start=(1, 3)),
    dict(edges=np.r_[np.arange(66.0), np.arange(65.0)], axis_col=(0, 1), axis_start=(0, 66, 131), panel_axes=[(0, 1)]),
    dict(axis_col=(2,)),
    dict(axis_col=(-1,)),
    dict(panel_axes=[(1, -1)]),
    dict(panel_axes=[(-1, -1)]),
    dict(panel_axes=[(0, 1)]),
    dict(panel_axes=[(0, -2)]),
    dict(null=("values",)),
    dict(null=("edges",)),
    dict(null=("axis_col",)),
    dict(null=("axis_start",)),
    dict(null=("panel_axes",)),
    dict(null=("logz",)),
    dict(null=("info",)),
    dict(null=("counts",)),
    dict(null=("outside_count",)),
    dict(null=("stats",)),
    dict(nsamples=0),
    dict(block_bytes=-1),
    dict(mode=2),
    dict(bootstrap=2),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    assert _raw(**args) == _abi.E_INVALID


def test_the_limits_themselves_are_accepted(gpu_required):
    assert _raw() == _abi.OK
    assert _raw(null=("mass",)) == _abi.OK and _raw(null=("outside",)) == _abi.OK and _raw(null=("mass", "outside")) == _abi.OK
    assert _raw(values=np.zeros((4, 64)), axis_col=(63,)) == _abi.OK
    assert _raw(edges=np.arange(256.0), axis_col=[0] * 128, axis_start=np.arange(0, 257, 2), panel_axes=[(127, -1)] * 256) == _abi.OK
    assert _raw(edges=np.arange(4097.0), axis_start=(0, 4097)) == _abi.OK
    assert _raw(edges=np.r_[np.arange(65.0), np.arange(65.0)], axis_col=(0, 1), axis_start=(0, 65, 130),
                panel_axes=[(0, 1), (1, 0), (1, 1)]) == _abi.OK
    # the table (2 bytes a row and axis) and one replicate (8 bytes a row, a bin and a panel): 2 * 4 + 8 * (4 + 2 + 1)
    assert _raw(block_bytes=63) == _abi.E_NOMEM and _raw(block_bytes=64) == _abi.OK


def test_what_merge_refuses_is_refused_and_a_short_block_bound_gives_nomem(gpu_required):
    logl, birth, run_start = _arrays(_ragged(7))
    values = _columns(logl.size, 7)
    axes, panels = [(0, np.linspace(-9.0, 9.0, 11)), (1, np.linspace(0.0, 4.0, 9))], [0, 1, (0, 1)]

    def call(logl=logl, birth=birth, rs=run_start, **kw):
        return marginals.marginals_arrays(values, logl, birth, rs, axes, panels, nsamples=4, device=0, **kw)

    lib = _abi.load()
    bad = logl.copy()
    bad[3] = np.nan
    out = [np.zeros(512) for _ in range(3)] + [np.zeros(512, np.int64) for _ in range(2)]
    edges = np.array([0.0, 1.0])
    rc = lib.rvll_marginal_replicates(0, _abi.as_dp(bad), _abi.as_dp(birth), logl.size, run_start.ctypes.data_as(_I64),
                                      run_start.size - 1, _abi.as_dp(values), 4, _abi.as_dp(edges),
                                      _abi.as_ip(np.zeros(1, np.int32)), np.array([0, 2], np.int64).ctypes.data_as(_I64), 1,
                                      _abi.as_ip(np.array([0, -1], np.int32)), 1, 2, 0, 1, 0, _abi.as_dp(out[0]), _abi.as_dp(out[1]),
                                      out[3].ctypes.data_as(_I64), out[4].ctypes.data_as(_I64), _abi.as_dp(out[2]), None, None, 0,
                                      None)
    assert rc == _abi.E_INVALID
    need = marginals.table_bytes(logl.size, 2) + marginals.replicate_bytes(logl.size, 10 + 8 + 80, 3)
    with pytest.raises(RvllError) as exc:
        call(block_bytes=need - 1)
    assert exc.value.code == _abi.E_NOMEM
    timing = {}
    exact = call(block_bytes=need, timing=timing)
    assert timing["blocks"] == 4
    roomy = call()
    assert all(np.array_equal(exact[k], roomy[k]) for k in exact)
