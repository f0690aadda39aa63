"""The insertion-index test of nested-sampling runs (Fowlie, Handley & Su 2020, "Nested sampling cross-checks using order
statistics").  If a sampler draws every new point from the prior restricted to L > L*, the new point's rank among the live
points is uniform on {0, ..., nlive - 1}; a KS test of the ranks finds a sampler that cannot reach part of the constrained
region or that stays too close to its start points, and a windowed test says when in the run that starts.  The numpy
definition below is the reference that the device entry (rvll_insertion_indexes, csrc/rvll_insertion.hip)
reproduces exactly.

Run r has rows (logl_i, birth_i) in any order (a result's `logl` and `logl_birth`), no NaN.  For a row j with birth
b = birth_j > -inf:

    live(j)  = { k in run r : birth_k <= b  and  logl_k > b }     the live set right after j was inserted
    n_at[j]  = |live(j)|
    index[j] = #{ k in live(j) : logl_k < logl_j }

Rows born at -inf (the initial live points) get index = n_at = -1.  A row with a finite birth and logl_j <= birth_j (the rare
end point that the exact redo of a wandering Kepler solve lowered to lstar or below) belongs to no live set; its index is 0 by
the formula and it is reported as off-contour.  Doubles are compared as doubles (-0.0 == +0.0).

The test (`test`) takes the inserted on-contour rows with n_at == nlive; the other inserted on-contour rows — born on a tied
contour such as a -1e30 plateau, for example — are reported as off-schedule.  Per run, with c_k the count of those rows whose
index is k and C_k the cumulative count over n rows:

    D = max_k |C_k / n - (k + 1) / nlive|,   p = scipy.stats.kstwo.sf(D, n)    (conservative for a discrete uniform)

The windowed test orders the same rows by (birth, row position), cuts them into consecutive windows of `window` rows (default
nlive; a trailing partial window is dropped) and computes D and p per window.  A run fails if p < alpha or if some window has
p < alpha / n_windows; the first such window is given by its birth contour (that of its first row) and by the number of deaths
before it, #{rows with logl <= that contour}.  D and p come from integer counts on the host, so the device and the definition
give identical records.
"""
import ctypes as C

import numpy as np

from . import _abi

_BLOCK_ELEMS = 1 << 22               # (row, row) pairs the numpy definition compares at a time


def check_args(logl, birth, run_start):
    """The arguments in canonical form — logl, birth float64 [N], run_start int64 [R + 1].  Raises ValueError where
    rvll_insertion_indexes returns RVLL_E_INVALID."""
    logl = np.ascontiguousarray(logl, dtype=np.float64).reshape(-1)
    birth = np.ascontiguousarray(birth, dtype=np.float64).reshape(-1)
    if birth.shape != logl.shape:
        raise ValueError("logl and birth need one entry per row")
    run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
    if run_start.shape[0] < 2:
        raise ValueError("need at least one run")
    if run_start[0] != 0 or run_start[-1] != logl.shape[0] or np.any(np.diff(run_start) < 0):
        raise ValueError("run_start must rise from 0 to the number of rows")
    if np.any(np.diff(run_start) >= 2 ** 31):
        raise ValueError("a run has 2^31 rows or more")
    if np.isnan(logl).any() or np.isnan(birth).any():
        raise ValueError("logl and birth must not hold NaN")
    return logl, birth, run_start


def _definition(logl, birth, run_start):
    index = np.full(logl.shape[0], -1, dtype=np.int32)
    n_at = np.full(logl.shape[0], -1, dtype=np.int32)
    for r in range(run_start.shape[0] - 1):
        a, e = int(run_start[r]), int(run_start[r + 1])
        ll, bb = logl[a:e], birth[a:e]
        ins = np.flatnonzero(bb > -np.inf)
        step = max(1, _BLOCK_ELEMS // max(1, e - a))
        for i0 in range(0, ins.shape[0], step):
            j = ins[i0:i0 + step]
            b = bb[j][:, None]
            live = (bb[None, :] <= b) & (ll[None, :] > b)
            n_at[a + j] = np.count_nonzero(live, axis=1)
            index[a + j] = np.count_nonzero(live & (ll[None, :] < ll[j][:, None]), axis=1)
    return index, n_at


def _device(logl, birth, run_start, device, timing):
    lib = _abi.load()
    index = np.empty(logl.shape[0], dtype=np.int32)
    n_at = np.empty(logl.shape[0], dtype=np.int32)
    t = _abi.InsertionTiming()
    _abi.check(lib.rvll_insertion_indexes(int(device), _abi.as_dp(logl), _abi.as_dp(birth), logl.shape[0],
                                          run_start.ctypes.data_as(C.POINTER(C.c_int64)), run_start.shape[0] - 1,
                                          _abi.as_ip(index), _abi.as_ip(n_at), C.byref(t)))
    if timing is not None:
        timing.update(kernel_ms=t.kernel_ms, total_ms=t.total_ms, rows=t.rows, launches=t.launches, threads=t.threads)
    return index, n_at


def indexes_arrays(logl, birth, run_start, device=None, timing=None):
    """(index, n_at), int32 [N] each, of R runs given as arrays: rows run_start[r] .. run_start[r + 1] of logl / birth are run r.
    device=None evaluates the numpy definition; device=k runs rvll_insertion_indexes on device k (timing: a dict that receives
    the call's rvll_insertion_timing)."""
    args = check_args(logl, birth, run_start)
    return _definition(*args) if device is None else _device(*args, device, timing)


def _stack(results):
    results = list(results)
    if not results:
        raise ValueError("need at least one result")
    for i, res in enumerate(results):
        if getattr(res, "logl_birth", None) is None:
            raise ValueError(f"result {i} has no birth contours (logl_birth)")
        if len(res.logl_birth) != len(res.logl):
            raise ValueError(f"result {i}: logl_birth and logl differ in length")
    logl = np.concatenate([np.asarray(res.logl, dtype=np.float64).reshape(-1) for res in results])
    birth = np.concatenate([np.asarray(res.logl_birth, dtype=np.float64).reshape(-1) for res in results])
    run_start = np.concatenate([[0], np.cumsum([len(res.logl) for res in results])]).astype(np.int64)
    return results, logl, birth, run_start


def indexes(results, device=None, timing=None):
    """Insertion indexes of finished runs (a list of NestedResult): a list of (index, n_at) pairs, one per result, in the order
    of its rows.  ValueError for a result without logl_birth."""
    results, logl, birth, run_start = _stack(results)
    index, n_at = indexes_arrays(logl, birth, run_start, device, timing)
    return [(index[run_start[r]:run_start[r + 1]], n_at[run_start[r]:run_start[r + 1]]) for r in range(len(results))]


def ks(counts):
    """(D, p) of the KS test of the rank counts c_k (k < nlive) against the uniform distribution on {0, ..., nlive - 1};
    (nan, nan) without rows."""
    from scipy.stats import kstwo
    counts = np.asarray(counts, dtype=np.int64)
    n = int(counts.sum())
    if n == 0:
        return float("nan"), float("nan")
    nl = counts.shape[0]
    d = float(np.max(np.abs(np.cumsum(counts) / n - np.arange(1, nl + 1) / nl)))
    return d, float(kstwo.sf(d, n))


def _run_record(logl, birth, index, n_at, nlive, window, alpha):
    ins = birth > -np.inf
    offc = ins & (logl <= birth)
    used = ins & ~offc & (n_at == nlive)
    counts = np.bincount(index[used], minlength=nlive)[:nlive]
    d, p = ks(counts)
    rec = {"nlive": nlive, "n": int(np.count_nonzero(used)), "off_schedule": int(np.count_nonzero(ins & ~offc & (n_at != nlive))),
           "off_contour": int(np.count_nonzero(offc)), "D": d, "pvalue": p, "counts": counts}
    rows = np.flatnonzero(used)
    rows = rows[np.lexsort((rows, birth[rows]))]             # by (birth, row position)
    w = int(window or nlive)
    nw = rows.shape[0] // w
    wd, wp = np.empty(nw), np.empty(nw)
    for i in range(nw):
        wd[i], wp[i] = ks(np.bincount(index[rows[i * w:(i + 1) * w]], minlength=nlive)[:nlive])
    bad = np.flatnonzero(wp < alpha / nw) if nw else np.zeros(0, dtype=np.int64)
    rec.update(window=w, windows=nw, window_D=wd, window_p=wp, failed=bool(p < alpha or bad.size > 0))
    if bad.size:
        contour = float(birth[rows[bad[0] * w]])
        rec.update(first_window=int(bad[0]), first_window_birth=contour,
                   first_window_deaths=int(np.count_nonzero(logl <= contour)))
    else:
        rec.update(first_window=None, first_window_birth=None, first_window_deaths=None)
    return rec


def test(results, device=None, window=None, alpha=0.01, timing=None):
    """The insertion-index test of finished runs (a list of NestedResult, each with nlive and logl_birth): {"runs": one record
    per run, "pooled": the counts of all runs tested together when every run has the same nlive, else None}.  A run's record
    holds n, off_schedule, off_contour, D, pvalue, the rank counts, the windowed test (window, windows, window_D, window_p),
    failed, and the first failing window (first_window, first_window_birth, first_window_deaths; None when no window fails).
    device=None: the numpy definition; device=k: rvll_insertion_indexes."""
    results, logl, birth, run_start = _stack(results)
    for i, res in enumerate(results):
        if getattr(res, "nlive", None) is None:
            raise ValueError(f"result {i} has no nlive")
    index, n_at = indexes_arrays(logl, birth, run_start, device, timing)
    recs = []
    for r, res in enumerate(results):
        sl = slice(run_start[r], run_start[r + 1])
        recs.append(_run_record(logl[sl], birth[sl], index[sl], n_at[sl], int(res.nlive), window, alpha))
    pooled = None
    if len({rec["nlive"] for rec in recs}) == 1:
        counts = np.sum([rec["counts"] for rec in recs], axis=0)
        d, p = ks(counts)
        pooled = {"nlive": recs[0]["nlive"], "n": int(counts.sum()), "off_schedule": sum(rec["off_schedule"] for rec in recs),
                  "off_contour": sum(rec["off_contour"] for rec in recs), "D": d, "pvalue": p, "counts": counts,
                  "failed": bool(p < alpha)}
    return {"runs": recs, "pooled": pooled}
