"""Pointwise predictive checks of merged nested-sampling runs with run-to-run error bars: per unit of the data — an epoch, a
night, an instrument — the in-sample log predictive density (lpd), its WAIC correction and the importance-sampling leave-one-out
value (LOO) (Gelman, Hwang & Vehtari 2014, "Understanding predictive information criteria for Bayesian models"; Vehtari, Gelman &
Gabry 2017, "Practical Bayesian model evaluation using leave-one-out cross-validation and WAIC"), for every replicate of the
merged run (merge.py: simulated shrinkage, optionally on top of a bootstrap of the runs).  They say which observations a
k-planet model fails to predict, and their sums score k against k + 1 without reference to the prior widths.  The numpy
definition below is the reference that the device entry (rvll_pointwise_replicates; csrc/rvll_pointwise.hip)
reproduces; on the device the replicated weights are reduced where they are written, by one fp64 product on the matrix units.

Table.  t [N, U]: the log-likelihood of unit u's data at row r (unit_loglik).  Per row and epoch
    l = -0.5 ln(2 pi) - ln(sqrt(var)) - res^2 / (2 var)
with res and var of model.residuals_batch — the operations of the reference's logL, so the sum of l over the epochs is the
row's log-L to rounding — and a unit's value is the sum of its epochs' l in rising epoch index.  A row with an invalid orbit has
-1e30 in every unit.

Shifts, once per call, from the expected-weight merged run (merge.merge_arrays, the numpy definition whatever the device):
    W    the rows with logwt >= -43.0 (62 ln 2: the "rows with weight" of the fixed-point reducers)
    c_u  the largest t[r, u] over W;   d_u  the smallest;   a_u = d_u + sum_W w (t - d_u) / sum_W w, the expected-weight mean

Per replicate s, with p the replicate's weights exp(logwt) in merged order (merge.replicates' own), P = sum p:
    lpd [s, u] = c_u + ln(sum p exp(min(t - c_u, 0)) / P)
    loo [s, u] = d_u - ln(sum p exp(min(d_u - t, 0)) / P)
    mean[s, u] = a_u + sum p (t - a_u) / P
    var [s, u] = sum p (t - a_u)^2 / P - (sum p (t - a_u) / P)^2
    waic = lpd - var
A replicate without mass (P = 0: a bootstrap of empty runs) has NaN in all four.

The two min(., 0) keep exp from overflowing on the rows outside W.  In lpd they change nothing that carries weight: a row with
t > c_u is outside W and counts as if t = c_u.  In loo they truncate the importance ratio 1 / p(y_u | theta) of a row outside W
at the largest ratio inside W: a weightless row with t < d_u counts with the ratio exp(-d_u), not its own.  truncated_rows[u]
counts those rows; loo_ess[u] is the Kish size (sum v)^2 / sum v^2 of v = p exp(min(d_u - t, 0)) over W on the expected-weight
run, the number of rows that carry the leave-one-out estimate.  Pareto smoothing of the ratios (PSIS, k-hat) is not done; loo_ess and
truncated_rows are the reliability diagnostics.

Every sum is over one unit's column alone, so a unit's results do not depend on the other units of the call, and splitting the
units into blocks (unit_block) changes no bit.
"""
import ctypes as C

import numpy as np

from . import _abi, merge
from .shrinkage import replicate_seeds

MAX_UNITS = 4096                         # units of one device call; more are split into blocks
MAX_ABS = 1e30                           # the largest |t|: (t - a)^2 stays finite
INVALID = -1e30                          # a row with an invalid orbit
WEIGHT_FLOOR = -43.0                     # logwt of the rows with weight (62 ln 2)
_LOG_2PI_HALF = 0.5 * np.log(2.0 * np.pi)
_BLOCK_ELEMS = 1 << 21                   # (replicate, row) elements the numpy definition holds at a time, per array
_SHIFT_ELEMS = 1 << 24                  # (row, unit) elements the host's shifts look at at a time
_M64 = 2 ** 64 - 1
_TILE_REPS = 64                          # replicates of one workgroup tile on the device


def slab_rows():
    """The rows of one slab of the device product (rvll_pointwise_slab_rows): a constant of the library."""
    rows = C.c_int32()
    _abi.check(_abi.load().rvll_pointwise_slab_rows(C.byref(rows)))
    return int(rows.value)


def _padded(nrows, units, slab):
    return -(-int(nrows) // 64) * 64, -(-(4 * int(units) + 1) // 64) * 64, -(-int(nrows) // slab)


def table_bytes(nrows, units, slab=16384):
    """Bytes of the device's per-call tables for `units` units: the operand B (rows rounded up to 64, 4 units + 1 columns rounded
    up to 64) and one tile of 64 replicates of partial sums.  block_bytes must hold them and at least one replicate_bytes."""
    rows, cols, slabs = _padded(nrows, units, slab)
    return 8 * (rows + _TILE_REPS * slabs) * cols


def replicate_bytes(nrows, units, slab=16384):
    """Bytes one replicate of a block takes on the device: its weights and its partial sums, one row a slab."""
    _, cols, slabs = _padded(nrows, units, slab)
    return 8 * (int(nrows) + slabs * cols)


def by_night(time, gap=0.5):
    """int64 [Ne]: a unit index per epoch in which epochs that follow each other in time by less than `gap` days share a unit;
    the units are numbered in rising time.  The epochs need not be sorted."""
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    if time.size < 1 or not np.isfinite(time).all():
        raise ValueError("need at least one finite epoch")
    order = np.argsort(time, kind="stable")
    unit = np.concatenate([[0], np.cumsum(np.diff(time[order]) >= gap)]).astype(np.int64)
    groups = np.empty(time.size, dtype=np.int64)
    groups[order] = unit
    return groups


def by_instrument(model):
    """int64 [Ne]: the instrument of every epoch of the model's table, one unit an instrument."""
    return np.asarray(model.table.inst_id, dtype=np.int64).copy()


def check_groups(groups, ne):
    """groups as int64 [Ne] with every value of 0 .. U - 1 in use; returns (groups, U)."""
    groups = np.ascontiguousarray(groups, dtype=np.int64).reshape(-1)
    if groups.shape[0] != ne:
        raise ValueError(f"groups has {groups.shape[0]} entries, the model {ne} epochs")
    units = int(groups.max()) + 1
    if groups.min() < 0 or np.unique(groups).size != units:
        raise ValueError("groups must use every value of 0 .. U - 1")
    return groups, units


def unit_loglik(model, thetas, groups=None, chunk=65536):
    """t [n, U]: the log-likelihood of every unit's data at every row of thetas [n, ndim] (module docstring).  groups: an int
    array [Ne] with values 0 .. U - 1, the unit of every epoch (by_night, by_instrument); None: every epoch its own unit.  The
    rows go through model.residuals_batch `chunk` at a time."""
    thetas = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    ne = int(np.asarray(model.table.time).shape[0])
    units = ne
    if groups is not None:
        groups, units = check_groups(groups, ne)
    out = np.empty((thetas.shape[0], units))
    for r0 in range(0, thetas.shape[0], int(chunk)):
        res, var = model.residuals_batch(thetas[r0:r0 + int(chunk)])
        with np.errstate(invalid="ignore", divide="ignore"):
            ell = -_LOG_2PI_HALF - np.log(np.sqrt(var)) - res ** 2 / (2 * var)
        if groups is None:
            t = ell
        else:
            t = np.zeros((ell.shape[0], units))
            for e in range(ne):                                   # left to right in rising epoch index
                t[:, groups[e]] += ell[:, e]
        t[np.isnan(res).any(axis=1)] = INVALID
        out[r0:r0 + t.shape[0]] = t
    return out


def check_table(table, logl):
    """table as float64 [N, U] (C-contiguous); raises ValueError where rvll_pointwise_replicates returns RVLL_E_INVALID for it
    (more than MAX_UNITS units are fine here: they go in blocks)."""
    table = np.asarray(table, dtype=np.float64)
    if table.ndim == 1:
        table = table[:, None]
    if table.ndim != 2 or table.shape[1] < 1:
        raise ValueError("table must be [rows, units] with at least one unit")
    table = np.ascontiguousarray(table)
    if table.shape[0] != np.asarray(logl).reshape(-1).shape[0]:
        raise ValueError(f"table has {table.shape[0]} rows, logl {np.asarray(logl).reshape(-1).shape[0]}")
    if not np.all(np.abs(table) <= MAX_ABS):
        raise ValueError("table values must be finite and at most 1e30 in size")
    return table


def shifts_of(table, logl, birth, run_start):
    """What a call computes once on the host from the expected-weight merged run: a dict with shifts [3, U] = (c, d, a), loo_ess
    [U] and truncated_rows int64 [U] (module docstring).  Only the rows of W are gathered.  Every unit is a contiguous row of its
    own while it is handled (numpy's pairwise sum of that row), so its numbers do not depend on the units next to it."""
    m = merge.merge_arrays(logl, birth, run_start)
    inside = m["logwt"] >= WEIGHT_FLOOR
    rows = m["order"][inside]                                     # the input rows of W, in merged order
    w = np.exp(m["logwt"][inside])
    wsum = w.sum()
    units = table.shape[1]
    shifts, ess, trunc = np.empty((3, units)), np.empty(units), np.empty(units, dtype=np.int64)
    step = max(1, _SHIFT_ELEMS // table.shape[0])
    for u0 in range(0, units, step):
        xw = np.ascontiguousarray(table[rows, u0:u0 + step].T)               # [units of the block, rows of W]
        c, d = xw.max(axis=1), xw.min(axis=1)
        shifts[:, u0:u0 + step] = c, d, d + ((xw - d[:, None]) * w).sum(axis=1) / wsum
        v = w * np.exp(np.minimum(d[:, None] - xw, 0.0))
        ess[u0:u0 + step] = v.sum(axis=1) ** 2 / (v * v).sum(axis=1)
        trunc[u0:u0 + step] = np.count_nonzero(table[:, u0:u0 + step] < d, axis=0)
    return dict(shifts=shifts, loo_ess=ess, truncated_rows=trunc)


def operand(tm, shifts):
    """The rows of the product's operand for the units of tm [N, U'] (merged order): float64 [4 U' + 1, N], ones, then E1, E2, z
    and z^2 per unit."""
    n, units = tm.shape
    out = np.empty((4 * units + 1, n))
    out[0] = 1.0
    for u in range(units):
        c, d, a = shifts[:, u]
        t = tm[:, u]
        z = t - a
        out[1 + 4 * u] = np.exp(np.minimum(t - c, 0.0))
        out[2 + 4 * u] = np.exp(np.minimum(d - t, 0.0))
        out[3 + 4 * u] = z
        out[4 + 4 * u] = z * z
    return out


def _reduce(p, bt, shifts, lpd, loo, mean, var):
    """One replicate and one block of units: the weights p [N] in merged order, the operand bt [4 U' + 1, N] and the block's
    shifts [3, U'].  Every row of bt is summed against p on its own (numpy's pairwise sum of N contiguous numbers), P among
    them."""
    with np.errstate(invalid="ignore", divide="ignore"):
        sums = (bt * p).sum(axis=1)
        total = sums[0]
        m1 = sums[3::4] / total
        lpd[:] = shifts[0] + np.log(sums[1::4] / total)
        loo[:] = shifts[1] - np.log(sums[2::4] / total)
        mean[:] = shifts[2] + m1
        var[:] = sums[4::4] / total - m1 * m1


def _definition(table, pre, logl, birth, run_start, nsamples, code, bootstrap, seed, unit_block):
    lay = merge._layout(logl, birth, run_start)
    N, R, units = logl.shape[0], lay["R"], table.shape[1]
    tm = table[lay["order"]]
    blocks = [(u0, min(units, u0 + unit_block)) for u0 in range(0, units, unit_block)]
    bts = [operand(tm[:, u0:u1], pre["shifts"][:, u0:u1]) for u0, u1 in blocks]
    seeds = replicate_seeds(seed, nsamples)
    logz, info = np.empty(nsamples), np.empty(nsamples)
    out = {k: np.empty((nsamples, units)) for k in ("lpd", "loo", "mean", "var")}
    step = max(1, _BLOCK_ELEMS // N)
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        w = merge.bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, _ = merge._block(lay, w, seeds[s0:s1], code == _abi.SHRINK_EXPECTED)
        for s in range(s0, s1):
            with np.errstate(invalid="ignore", under="ignore"):
                p = np.exp(logw[s - s0] - logz[s])
            for (u0, u1), bt in zip(blocks, bts):
                _reduce(p, bt, pre["shifts"][:, u0:u1], *(out[k][s, u0:u1] for k in ("lpd", "loo", "mean", "var")))
    return logz, info, out


def _device(table, pre, logl, birth, run_start, nsamples, code, bootstrap, seed, unit_block, device, block_bytes, timing):
    lib = _abi.load()
    N, R, units = logl.shape[0], run_start.shape[0] - 1, table.shape[1]
    logz, info = np.empty(nsamples), np.empty(nsamples)
    out = {k: np.empty((nsamples, units)) for k in ("lpd", "loo", "mean", "var")}
    total = None
    for u0 in range(0, units, unit_block):
        u1 = min(units, u0 + unit_block)
        tab = np.ascontiguousarray(table[:, u0:u1])
        sh = np.ascontiguousarray(pre["shifts"][:, u0:u1])
        part = {k: np.empty((nsamples, u1 - u0)) for k in out}
        t = _abi.PointwiseTiming()
        _abi.check(lib.rvll_pointwise_replicates(
            int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(C.POINTER(C.c_int64)), R,
            _abi.as_dp(tab), u1 - u0, _abi.as_dp(sh), nsamples, code, 1 if bootstrap else 0, int(seed) & _M64,
            _abi.as_dp(logz), _abi.as_dp(info), _abi.as_dp(part["lpd"]), _abi.as_dp(part["loo"]), _abi.as_dp(part["mean"]),
            _abi.as_dp(part["var"]), int(block_bytes or 0), C.byref(t)))
        for k in out:
            out[k][:, u0:u1] = part[k]
        now = {name: getattr(t, name) for name, _ in t._fields_}
        if total is None:
            total = dict(now, unit_blocks=1)
        else:                                                     # the times, the columns and the launches add up over the unit blocks
            for name in ("kernel_ms", "total_ms", "setup_ms", "weights_ms", "reduce_ms", "columns", "launches", "blocks"):
                total[name] += now[name]
            total["unit_blocks"] += 1
    if timing is not None:
        timing.update(total)
    return logz, info, out


def _unit_block(unit_block, units, nrows, block_bytes):
    if unit_block is not None:
        if int(unit_block) < 1:
            raise ValueError("unit_block must be at least 1")
        return min(int(unit_block), MAX_UNITS, units)
    ub = min(units, MAX_UNITS)
    if block_bytes:                                               # the largest block whose operand fits beside one replicate
        while ub > 1 and table_bytes(nrows, ub) + replicate_bytes(nrows, ub) > int(block_bytes):
            ub = (ub + 1) // 2
    return ub


def pointwise_arrays(table, logl, birth, run_start, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None,
                     block_bytes=None, unit_block=None, timing=None):
    """The pointwise checks of `table` (float64 [N, U] in input row order, finite, at most 1e30 in size) over nsamples replicates
    of the merged run of the runs (logl, birth, run_start) as merge.replicates_arrays takes them: a dict with lpd, loo, mean, var
    and waic = lpd - var, each [S, U]; logz [S] and information [S], the bits of merge.replicates_arrays; and from the
    expected-weight run loo_ess [U], truncated_rows [U] and shifts [3, U] (module docstring).  device=None evaluates the numpy
    definition; device=k runs rvll_pointwise_replicates on device k (block_bytes bounds table_bytes(N, U') plus the block of
    replicates, replicate_bytes(N, U') each; timing: a dict that receives the call's rvll_pointwise_timing, summed over the unit
    blocks).  unit_block: the units of one block U' (default: all, at most 4096, or as many as block_bytes holds beside one
    replicate); the same seed gives the same replicates and the units are independent, so the split changes no bit."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    table = check_table(table, logl)
    return _arrays(table, shifts_of(table, logl, birth, run_start), logl, birth, run_start, nsamples, code, seed, bootstrap,
                   device, block_bytes, unit_block, timing)


def _arrays(table, pre, logl, birth, run_start, nsamples, code, seed, bootstrap, device, block_bytes, unit_block, timing):
    """pointwise_arrays on checked arguments, with what shifts_of returned for them."""
    ub = _unit_block(unit_block, table.shape[1], logl.shape[0], None if device is None else block_bytes)
    if device is None:
        logz, info, out = _definition(table, pre, logl, birth, run_start, nsamples, code, bootstrap, seed, ub)
    else:
        logz, info, out = _device(table, pre, logl, birth, run_start, nsamples, code, bootstrap, seed, ub, device, block_bytes,
                                  timing)
    return dict(out, waic=out["lpd"] - out["var"], logz=logz, information=info, loo_ess=pre["loo_ess"],
                truncated_rows=pre["truncated_rows"], shifts=pre["shifts"])


def _samples(results):
    results, logl, birth, run_start = merge._stack(results)
    for i, res in enumerate(results):
        if getattr(res, "samples", None) is None or len(res.samples) != len(res.logl):
            raise ValueError(f"result {i} has no samples for its rows")
    samples = np.concatenate([np.asarray(res.samples, dtype=np.float64).reshape(len(res.logl), -1) for res in results])
    return samples, logl, birth, run_start


def loo(results, model, groups=None, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, block_bytes=None,
        unit_block=None, timing=None, chunk=65536, table=None):
    """The pointwise checks of finished runs (a list of NestedResult with samples and logl_birth, stacked as merge.merge stacks
    them) under `model` (a GpuRVModel: unit_loglik evaluates its residuals at every row).  groups: None for one unit an epoch,
    or by_night(model.table.time) / by_instrument(model) / any int array [Ne].  Returns a dict: per unit lpd, waic and loo [U]
    from the merged run's expected weights (mode="expected", no bootstrap, one replicate), each with *_err, *_min and *_max,
    the standard deviation and the range over nsamples replicates (mode / bootstrap / seed); their sums over the units as
    lpd_total, waic_total, loo_total with the same three; p_waic [U] (the variance of the unit's log-likelihood) and
    p_waic_total; loo_ess and truncated_rows [U]; units; table, the [N, U] table; replicates, the pointwise_arrays dict.
    table: what unit_loglik(model, samples, groups) returned for these results, to spare evaluating it again."""
    samples, logl, birth, run_start = _samples(results)
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    table = check_table(unit_loglik(model, samples, groups, chunk) if table is None else table, logl)
    pre = shifts_of(table, logl, birth, run_start)
    point = _arrays(table, pre, logl, birth, run_start, 1, _abi.SHRINK_EXPECTED, seed, False, device, block_bytes, unit_block, None)
    reps = _arrays(table, pre, logl, birth, run_start, nsamples, code, seed, bootstrap, device, block_bytes, unit_block, timing)
    out = dict(units=table.shape[1], nsamples=int(nsamples), table=table, replicates=reps, p_waic=point["var"][0],
               p_waic_total=float(point["var"][0].sum()), loo_ess=point["loo_ess"], truncated_rows=point["truncated_rows"])
    for key in ("lpd", "waic", "loo"):
        out[key] = point[key][0]
        out[key + "_err"] = np.std(reps[key], axis=0)
        out[key + "_min"] = np.min(reps[key], axis=0)
        out[key + "_max"] = np.max(reps[key], axis=0)
        tot = reps[key].sum(axis=1)
        out[key + "_total"] = float(point[key][0].sum())
        out[key + "_total_err"] = float(np.std(tot))
        out[key + "_total_min"] = float(np.min(tot))
        out[key + "_total_max"] = float(np.max(tot))
    return out


def compare(a, b):
    """Two loo(...) results on the same units (two models of one data set): a dict with elpd_diff = a's loo_total - b's (positive:
    a predicts the held-out data better), err_replicates = sqrt(a's loo_total_err^2 + b's), the run-to-run error of the
    difference, err_units = sqrt(U var_u(Delta_u)) with Delta_u = loo_a[u] - loo_b[u] and var the mean square about the mean,
    the between-unit standard error of the sum, and delta, Delta_u itself."""
    if a["units"] != b["units"]:
        raise ValueError(f"the results have {a['units']} and {b['units']} units")
    delta = np.asarray(a["loo"]) - np.asarray(b["loo"])
    return dict(elpd_diff=float(a["loo_total"] - b["loo_total"]),
                err_replicates=float(np.sqrt(a["loo_total_err"] ** 2 + b["loo_total_err"] ** 2)),
                err_units=float(np.sqrt(delta.size * np.var(delta))), delta=delta)
