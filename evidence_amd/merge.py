"""Merging nested-sampling runs by their birth contours (Skilling 2006; Higson et al. 2018, "Sampling errors in nested sampling
parameter estimation"; dynesty's merge_runs): R finished runs of one model become one run whose live count varies from death to
death, with its evidence, its posterior weights and — by simulated shrinkage on top of a bootstrap of the runs — an error bar that
holds the run-to-run scatter.  The numpy definition below is the reference that the device entries (rvll_merge_runs,
rvll_merge_replicates; csrc/rvll_merge.hip) reproduce.

The input is R runs of rows (logl, birth) in any order (a result's `logl` and `logl_birth`); no NaN, no infinite log-L.

    order        all rows sorted stably by log-L; ties go by run, then by the row's position in its run.  Row i of the merged
                 run has log-L L_i, birth b_i and run rho_i.
    off-contour  a row with logl <= birth (the rare end point that the exact redo lowered; insertion.py) counts with the birth
                 nextafter(L_i, -inf).  merge_arrays reports how many there are.
    live count   with multiplicities w_r (1 each without the bootstrap):
                     n_i = sum_{k: b_k < L_i} w_{rho_k} - sum_{k < i} w_{rho_k}
                 Row i stands for w = w_{rho_i} deaths in a row, at the counts n_i, n_i - 1, ..., n_i - w + 1; rows with w = 0 take
                 no part (weight -inf).  n_i >= w always: the rows k >= i born below L_i include row i itself.
    shrinkage    "expected":  Delta_i = -sum_{q<w} 1 / (n_i - q)
                 "random":    Delta_i =  sum_{q<w} log(u_c) / (n_i - q),   u_c = 1 - uniform01(seed_s, c),
                              c = sum_{k<i} w_{rho_k} + q  (the copies that died before)
                 both summed in the order q = 0, 1, ..., w - 1;  seed_s = seed + s * SEED_MUL mod 2^64 (as shrinkage.py).
    weights      logX_i = the running sum of Delta (logX_{-1} = 0), logw_i = (L_i + logX_{i-1}) + log(-expm1(Delta_i)),
                 lnZ = logsumexp(logw), H = sum_i e^{logw_i - lnZ} L_i - lnZ (0 without weight), logwt = logw - lnZ.
    bootstrap    w_r = how often r comes up among the R draws floor(uniform01(seed_s ^ BOOT_XOR, t) * R), t < R.

This is the thread convention: the final live points of a run die one by one at the counts m, m - 1, ..., 1, and the volume left
after the last death is dropped.  The drivers give their final live points logX_last - log m each instead, so merge([r]).logz
does not equal r.logz bit for bit (the two differ by far less than the run's shrinkage error).  H is the information of every
row, the merged run having no final live set.

The running sum logX is taken in extended precision (np.longdouble) and rounded once per row, and the device's tiled scan
carries a compensated sum between tiles: both stay within an ulp or two of the exact running sum, so the device and the
definition agree to round-off (the tests hold them to 1e-12 relative), not always to the bit (DESIGN §4j says why).  The live counts, the order and the
off-contour count are integers and agree exactly.
"""
import ctypes as C

import numpy as np

from . import _abi
from .nested import NestedResult
from .shrinkage import MODES, replicate_seeds

BOOT_XOR = 0x5851F42D4C957F2D        # the bootstrap draws of replicate s use the seed seed_s ^ BOOT_XOR
MAX_ROWS = 2 ** 30 - 1               # the device's event stream (2 N entries) keeps 32-bit positions
MAX_BOOT_RUNS = 8192                 # bootstrap multiplicities live in LDS on the device: 4 bytes a run
_BLOCK_ELEMS = 1 << 21               # (replicate, row) elements the numpy definition holds at a time, per array
_M64 = 2 ** 64 - 1


def uniform_at(seeds, counters):
    """float64: uniform01(seeds, counters) of rvll_math.h elementwise (broadcasting), bit for bit."""
    with np.errstate(over="ignore"):
        z = np.asarray(seeds, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(counters, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 1.1102230246251565404e-16


def check_args(logl, birth, run_start, nsamples=1, mode="expected", bootstrap=False):
    """The arguments in canonical form — logl, birth float64 [N], run_start int64 [R + 1], nsamples, mode code.  Raises
    ValueError where rvll_merge_runs / rvll_merge_replicates return RVLL_E_INVALID."""
    logl = np.ascontiguousarray(logl, dtype=np.float64).reshape(-1)
    birth = np.ascontiguousarray(birth, dtype=np.float64).reshape(-1)
    if birth.shape != logl.shape:
        raise ValueError("logl and birth need one entry per row")
    run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
    if run_start.shape[0] < 2:
        raise ValueError("need at least one run")
    if run_start[0] != 0 or run_start[-1] != logl.shape[0] or np.any(np.diff(run_start) < 0):
        raise ValueError("run_start must rise from 0 to the number of rows")
    if logl.shape[0] < 1 or logl.shape[0] > MAX_ROWS:
        raise ValueError(f"need 1 to {MAX_ROWS} rows")
    if np.isnan(birth).any():
        raise ValueError("birth must not hold NaN")
    if not np.isfinite(logl).all():
        raise ValueError("log-L must be finite: no NaN, no -inf or +inf rows")
    if int(nsamples) < 1 or int(nsamples) > 2 ** 31 - 1:
        raise ValueError("nsamples must be in [1, 2^31)")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    if bootstrap and run_start.shape[0] - 1 > MAX_BOOT_RUNS:
        raise ValueError(f"the run bootstrap takes at most {MAX_BOOT_RUNS} runs")
    return logl, birth, run_start, int(nsamples), MODES[mode]


def _layout(logl, birth, run_start):
    """The merged order and everything a replicate needs that does not depend on it."""
    R = run_start.shape[0] - 1
    run = np.repeat(np.arange(R, dtype=np.int32), np.diff(run_start))
    off = logl <= birth
    beff = np.where(off, np.nextafter(logl, -np.inf), birth)
    order = np.argsort(logl, kind="stable")                  # rows of a run are contiguous: ties go by (run, position)
    border = np.argsort(beff, kind="stable")
    sb = beff[border]
    L = logl[order]
    return dict(order=order, L=L, rho=run[order], rb=run[border], cntb=np.searchsorted(sb, L, side="left"),
                off_contour=int(np.count_nonzero(off)), R=R)


def bootstrap_weights(seeds, R):
    """int64 [len(seeds), R]: the run multiplicities w_r of the replicates with seeds seed_s."""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1)
    u = uniform_at((seeds ^ np.uint64(BOOT_XOR))[:, None], np.arange(R, dtype=np.uint64)[None, :])
    draw = np.minimum(np.floor(u * R).astype(np.int64), R - 1)
    flat = draw + (np.arange(seeds.shape[0], dtype=np.int64) * R)[:, None]
    return np.bincount(flat.reshape(-1), minlength=seeds.shape[0] * R).reshape(seeds.shape[0], R)


def _block(lay, w, seeds, expected):
    """One block of replicates with multiplicities w [S_b, R]: (logz, information, logw [S_b, N], n [S_b, N])."""
    Sb, N = w.shape[0], lay["L"].shape[0]
    wd = w[:, lay["rho"]]                                    # the multiplicity of every row
    pb = np.concatenate([np.zeros((Sb, 1), np.int64), np.cumsum(w[:, lay["rb"]], axis=1)], axis=1)
    pd = np.cumsum(wd, axis=1) - wd                           # the copies that died before row i
    n = np.take_along_axis(pb, np.broadcast_to(lay["cntb"], (Sb, N)), axis=1) - pd
    delta = np.zeros((Sb, N))
    for q in range(int(wd.max()) if wd.size else 0):
        act = wd > q
        nn = np.where(act, n - q, 1).astype(np.float64)
        if expected:
            term = -1.0 / nn
        else:
            term = np.log(1.0 - uniform_at(seeds[:, None], pd + q)) / nn
        delta += np.where(act, term, 0.0)
    lx = np.cumsum(delta.astype(np.longdouble), axis=1)
    logx_prev = np.concatenate([np.zeros((Sb, 1)), lx[:, :-1].astype(np.float64)], axis=1)
    with np.errstate(divide="ignore"):
        logw = np.where(wd > 0, (lay["L"] + logx_prev) + np.log(-np.expm1(delta)), -np.inf)
    top = np.max(logw, axis=1)
    fin = top > -np.inf
    safe = np.where(fin, top, 0.0)
    e = np.where(logw > -np.inf, np.exp(logw - safe[:, None]), 0.0)
    s = np.sum(e, axis=1)
    a = np.sum(np.where(e > 0, e * lay["L"], 0.0), axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        lnz = np.where(fin, safe + np.log(np.where(fin, s, 1.0)), -np.inf)
        info = np.where(fin, a / np.where(fin, s, 1.0) - lnz, 0.0)
    return lnz, info, logw, n


def _definition(logl, birth, run_start, nsamples, mode, bootstrap, seed, return_logwt):
    lay = _layout(logl, birth, run_start)
    N, R = logl.shape[0], lay["R"]
    seeds = replicate_seeds(seed, nsamples)
    logz, info = np.empty(nsamples), np.empty(nsamples)
    logwt = np.empty((nsamples, N)) if return_logwt else None
    step = max(1, _BLOCK_ELEMS // N)
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        w = bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, n = _block(lay, w, seeds[s0:s1], mode == _abi.SHRINK_EXPECTED)
        if logwt is not None:
            logwt[s0:s1] = logw - logz[s0:s1, None]
    return lay, logz, info, logwt, n


def _device_merge(logl, birth, run_start, device, timing):
    lib = _abi.load()
    N, R = logl.shape[0], run_start.shape[0] - 1
    order, nlive = np.empty(N, np.int64), np.empty(N, np.int64)
    logz, info, logwt = C.c_double(), C.c_double(), np.empty(N)
    n_off = C.c_int64()
    t = _abi.MergeTiming()
    _abi.check(lib.rvll_merge_runs(int(device), _abi.as_dp(logl), _abi.as_dp(birth), N,
                                   run_start.ctypes.data_as(C.POINTER(C.c_int64)), R,
                                   order.ctypes.data_as(C.POINTER(C.c_int64)), nlive.ctypes.data_as(C.POINTER(C.c_int64)),
                                   C.byref(logz), C.byref(info), _abi.as_dp(logwt), C.byref(n_off), C.byref(t)))
    _timing(timing, t)
    return order, nlive, logz.value, info.value, logwt, int(n_off.value)


def _timing(timing, t):
    if timing is not None:
        timing.update(kernel_ms=t.kernel_ms, total_ms=t.total_ms, rows=t.rows, elements=t.elements, launches=t.launches,
                      threads=t.threads)


def merge_arrays(logl, birth, run_start, device=None, timing=None):
    """The merged run of R runs given as arrays (rows run_start[r] .. run_start[r + 1] of logl / birth are run r, in any order):
    a dict with order (int64 [N], the input row of every merged row), nlive_row (int64 [N], n_i), run_index (int32 [N], rho_i),
    logz, information, logwt (float64 [N], in merged order; expected shrinkage) and off_contour (the rows counted with the birth
    nextafter(logl, -inf)).  device=None evaluates the numpy definition; device=k runs rvll_merge_runs on device k (timing: a dict
    that receives the call's rvll_merge_timing)."""
    logl, birth, run_start, _, _ = check_args(logl, birth, run_start)
    R = run_start.shape[0] - 1
    run = np.repeat(np.arange(R, dtype=np.int32), np.diff(run_start))
    if device is None:
        lay, logz, info, logwt, n = _definition(logl, birth, run_start, 1, _abi.SHRINK_EXPECTED, False, 0, True)
        order, nlive, logz, info, logwt, n_off = lay["order"].astype(np.int64), n[0], float(logz[0]), float(info[0]), logwt[0], \
            lay["off_contour"]
    else:
        order, nlive, logz, info, logwt, n_off = _device_merge(logl, birth, run_start, device, timing)
    return dict(order=order, nlive_row=nlive, run_index=run[order], logz=logz, information=info, logwt=logwt, off_contour=n_off)


def _device_replicates(logl, birth, run_start, nsamples, mode, bootstrap, seed, return_logwt, device, block_bytes, timing):
    lib = _abi.load()
    N, R = logl.shape[0], run_start.shape[0] - 1
    logz, info = np.empty(nsamples), np.empty(nsamples)
    logwt = np.empty((nsamples, N)) if return_logwt else None
    t = _abi.MergeTiming()
    _abi.check(lib.rvll_merge_replicates(
        int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(C.POINTER(C.c_int64)), R, nsamples, mode,
        1 if bootstrap else 0, int(seed) & _M64, _abi.as_dp(logz), _abi.as_dp(info),
        _abi.as_dp(logwt) if logwt is not None else None, int(block_bytes or 0), C.byref(t)))
    _timing(timing, t)
    return logz, info, logwt


def replicates_arrays(logl, birth, run_start, nsamples=1000, seed=0, mode="random", bootstrap=True, return_logwt=False,
                      device=None, block_bytes=None, timing=None):
    """Replicates of the merged run of R runs given as arrays: (logz [S], information [S]) and, with return_logwt, the weights
    [S, N] in merged order as a third element.  Replicate s uses seed_s = seed + s * SEED_MUL: its shrinkage draws, and with
    bootstrap=True its run multiplicities.  mode="expected", bootstrap=False gives merge_arrays' logz in every replicate.
    device=None: the numpy definition; device=k: rvll_merge_replicates (block_bytes bounds the device block of weights, default
    512 MiB; timing: a dict that receives the call's rvll_merge_timing)."""
    logl, birth, run_start, nsamples, code = check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    if device is None:
        _, logz, info, logwt, _ = _definition(logl, birth, run_start, nsamples, code, bootstrap, seed, return_logwt)
    else:
        logz, info, logwt = _device_replicates(logl, birth, run_start, nsamples, code, bootstrap, seed, return_logwt, device,
                                               block_bytes, timing)
    return (logz, info, logwt) if return_logwt else (logz, info)


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


def merge(results, device=None, timing=None):
    """One NestedResult from finished runs (a list of NestedResult with logl_birth): the rows of all runs in merged order
    (samples, logl, logwt, logl_birth), logz and information by the expected shrinkage, nlive_row (the live count n_i at every
    death) and run_index (the result every row comes from).  logzerr is sqrt(H / n_0), n_0 = nlive_row[0] the live count at the
    first death (the runs' initial live points together); niter counts every row, all of which die.  nlive / kbatch are None:
    the merged run has no fixed schedule (shrinkage.replicates does not take it; use replicates here).  merge([r]).logz differs
    from r.logz by the convention for the final live points (module docstring).  device=None: the numpy definition; device=k:
    rvll_merge_runs.  merge_arrays gives the number of off-contour rows as well."""
    results, logl, birth, run_start = _stack(results)
    m = merge_arrays(logl, birth, run_start, device, timing)
    order = m["order"]
    samples = None
    if all(getattr(res, "samples", None) is not None and len(res.samples) == len(res.logl) for res in results):
        samples = np.concatenate([np.asarray(res.samples).reshape(len(res.logl), -1) for res in results])[order]
    info = float(m["information"])
    return NestedResult(logz=float(m["logz"]), logzerr=float(np.sqrt(max(info, 0.0) / m["nlive_row"][0])), niter=int(logl.shape[0]),
                        ncall=int(sum(int(getattr(res, "ncall", 0) or 0) for res in results)), information=info,
                        samples=samples, logl=logl[order], logwt=m["logwt"], logl_birth=birth[order],
                        nlive_row=m["nlive_row"], run_index=m["run_index"])


def replicates(results, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, return_logwt=False, block_bytes=None,
               timing=None):
    """Replicates of the merged run of finished runs (a list of NestedResult with logl_birth): (logz [S], information [S]), and
    with return_logwt the weights [S, N] in the merged order of merge(results).  bootstrap=True resamples the runs with
    replacement in every replicate (Higson et al. 2018 §4), on top of the simulated shrinkage; bootstrap=False redraws the
    shrinkage alone.  device=None: the numpy definition; device=k: rvll_merge_replicates."""
    _, logl, birth, run_start = _stack(results)
    return replicates_arrays(logl, birth, run_start, nsamples, seed, mode, bootstrap, return_logwt, device, block_bytes, timing)


def logz_error(results, nsamples=1000, seed=0, device=None, **kw):
    """The standard deviation of ln Z over the merged run's replicates (with the run bootstrap unless bootstrap=False)."""
    return float(np.std(replicates(results, nsamples, seed, device=device, **kw)[0]))
