"""Simulated shrinkage ("simulated weights", Skilling 2006; Higson et al. 2018): the statistical scatter of ln Z, H and
the posterior weights of a finished nested-sampling run, from the run's own log-L sequence.  The numpy definition below
 is the reference that the device entry (rvll_shrinkage_replicates, csrc/rvll_shrinkage.hip) reproduces.

Run r has log-L values logl (the result's `logl`: the n_dead dead points in death order, then the m final live points),
nlive live points and kbatch deaths per iteration (run_nested: kbatch = 1).  Replicate s of run r:

    n_j      = nlive - (j mod kbatch)                        live count while death j (0 <= j < n_dead) dies (_deaths)
    seed_rs  = seeds[r] + s * 0xD1B54A32D192ED03  (mod 2^64)
    u_j      = 1 - uniform01(seed_rs, j)                     the splitmix64 draw of rvll_math.h, in (0, 1]
    log t_j  = log(u_j) / n_j                                t_j ~ Beta(n_j, 1), the shrinkage of death j
               (mode "expected": log t_j = -1 / n_j, the drivers' own schedule)
    logX_j   = logX_{j-1} + log t_j,  logX_{-1} = 0
    logw_j   = logl_j + logX_{j-1} + log(-expm1(log t_j))    dead point j
    logw_i   = logX_last - log(m) + logl_i                   final live point i (the drivers' convention)
    lnZ_s    = logsumexp(logw) over all rows
    H_s      = sum_dead exp(logw_j - lnZd) logl_j - lnZd,    lnZd = logsumexp(logw_j) over the dead points
    logwt_s  = logw - lnZ_s

H is the information of the dead points, as every driver reports it (`information`); it is 0 without dead points (or
when none carries weight).  A row whose logw is -inf takes no part in the sums.  With the expected shrinkage this gives the
driver's logz, information and logwt to round-off, which checks that the schedule is the one the run used.

The replicate seeds are spaced by 0xD1B54A32D192ED03, which is not a small multiple of splitmix64's own index step
0x9E3779B97F4A7C15: the counter streams of two replicates s < 200000 of one run lie >= 9·10^13 indices apart.
`replicates(..., seed=k)` gives run r the seed keep_words(k, R)[r] (clustering.keep_words: a splitmix64 word); pass a
sequence of R seeds to choose them yourself — a run's replicates depend only on its own log-L, schedule and seed.
"""
import ctypes as C

import numpy as np

from . import _abi
from .clustering import keep_words

SEED_MUL = 0xD1B54A32D192ED03        # seed of replicate s: seeds[r] + s * SEED_MUL
MODES = {"random": _abi.SHRINK_RANDOM, "expected": _abi.SHRINK_EXPECTED}
_M64 = 2 ** 64 - 1
_BLOCK_ELEMS = 1 << 21               # (replicate, row) elements the numpy definition holds at a time, per array


def _as_seeds(seeds):
    """uint64 [n] from an int or a sequence of ints, each taken mod 2^64 (no trip through float64)."""
    if isinstance(seeds, np.ndarray) and seeds.dtype.kind in "ui":
        return seeds.reshape(-1).astype(np.uint64)
    if np.ndim(seeds) == 0:
        seeds = [seeds]
    return np.array([int(s) & _M64 for s in seeds], dtype=np.uint64)


def uniform01(seeds, n):
    """float64 [len(seeds), n]: uniform01(seeds[i], j) of rvll_math.h for j < n, bit for bit."""
    seeds = _as_seeds(seeds)
    with np.errstate(over="ignore"):
        z = seeds[:, None] + np.uint64(0x9E3779B97F4A7C15) * (np.arange(n, dtype=np.uint64) + np.uint64(1))[None, :]
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 1.1102230246251565404e-16


def replicate_seeds(seed, nsamples):
    """uint64 [nsamples]: seed + s * SEED_MUL mod 2^64."""
    with np.errstate(over="ignore"):
        return np.uint64(int(seed) & _M64) + np.uint64(SEED_MUL) * np.arange(nsamples, dtype=np.uint64)


def live_counts(n_dead, nlive, kbatch):
    """int64 [n_dead]: n_j = nlive - (j mod kbatch)."""
    return nlive - np.arange(n_dead, dtype=np.int64) % kbatch


def check_args(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode):
    """The arguments in canonical form — logl float64 [N], run_start int64 [R + 1], n_dead int64 [R], nlive, kbatch int32 [R],
    seeds uint64 [R], nsamples, mode code.  Raises ValueError where rvll_shrinkage_replicates returns RVLL_E_INVALID."""
    logl = np.ascontiguousarray(logl, dtype=np.float64).reshape(-1)
    run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
    R = run_start.shape[0] - 1
    if R < 0 or run_start[0] != 0 or run_start[-1] != logl.shape[0] or np.any(np.diff(run_start) < 0):
        raise ValueError("run_start must rise from 0 to the number of log-L rows")
    n_dead = np.ascontiguousarray(n_dead, dtype=np.int64).reshape(-1)
    nlive = np.ascontiguousarray(nlive, dtype=np.int64).reshape(-1)
    kbatch = np.ascontiguousarray(kbatch, dtype=np.int64).reshape(-1)
    if not n_dead.shape[0] == nlive.shape[0] == kbatch.shape[0] == R:
        raise ValueError("n_dead, nlive and kbatch need one entry per run")
    if np.any(n_dead < 0):
        raise ValueError("n_dead must be >= 0")
    if np.any(kbatch < 1) or np.any(kbatch >= nlive) or np.any(nlive > 2 ** 31 - 1):
        raise ValueError("need 1 <= kbatch < nlive < 2^31")
    if np.any(n_dead % kbatch != 0):
        raise ValueError("n_dead must be a multiple of kbatch: every iteration kills kbatch points")
    if np.any(np.diff(run_start) - n_dead < 1):
        raise ValueError("every run needs at least one final live row (m >= 1) after its n_dead dead rows")
    seeds = _as_seeds(seeds)
    if seeds.shape[0] != R:
        raise ValueError("seeds needs one entry per run")
    if int(nsamples) < 1 or int(nsamples) > 2 ** 31 - 1:
        raise ValueError("nsamples must be in [1, 2^31)")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}")
    return logl, run_start, n_dead, nlive.astype(np.int32), kbatch.astype(np.int32), seeds, int(nsamples), MODES[mode]


def _one_run(ll, n_dead, nlive, kbatch, seed, nsamples, expected, logwt):
    """The definition for one run: (logz [S], information [S]); fills logwt [S, rows] when it is given."""
    ll_dead, ll_live = ll[:n_dead], ll[n_dead:]
    m = ll_live.shape[0]
    n_j = live_counts(n_dead, nlive, kbatch).astype(np.float64)
    logz, info = np.empty(nsamples), np.zeros(nsamples)
    step = max(1, _BLOCK_ELEMS // max(1, ll.shape[0]))
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        if expected:
            logt = np.broadcast_to(-1.0 / n_j, (s1 - s0, n_dead))
        else:
            logt = np.log(1.0 - uniform01(replicate_seeds(seed, nsamples)[s0:s1], n_dead)) / n_j
        logx = np.cumsum(logt, axis=1)
        logx_prev = np.concatenate([np.zeros((s1 - s0, 1)), logx[:, :-1]], axis=1)
        with np.errstate(divide="ignore"):
            logw_dead = (ll_dead + logx_prev) + np.log(-np.expm1(logt))
        logx_last = logx[:, -1] if n_dead else np.zeros(s1 - s0)
        logw_live = (logx_last - np.log(m))[:, None] + ll_live
        lnz_dead, a_dead, s_dead = _reduce(logw_dead, ll_dead)
        lnz_live = _reduce(logw_live, None)[0]
        lnz = np.logaddexp(lnz_dead, lnz_live)
        logz[s0:s1] = lnz
        ok = np.isfinite(lnz_dead)
        with np.errstate(invalid="ignore", divide="ignore"):
            info[s0:s1] = np.where(ok, a_dead / np.where(ok, s_dead, 1.0) - lnz_dead, 0.0)
        if logwt is not None:
            logwt[s0:s1, :n_dead] = logw_dead - lnz[:, None]
            logwt[s0:s1, n_dead:] = logw_live - lnz[:, None]
    return logz, info


def _reduce(logw, ll):
    """Per row: (logsumexp of logw, sum of e * ll, sum of e) with e = exp(logw - max); rows without a finite max give
    (-inf, 0, 0).  -inf entries take no part."""
    if logw.shape[1] == 0:
        z = np.zeros(logw.shape[0])
        return np.full(logw.shape[0], -np.inf), z, z
    top = np.max(logw, axis=1)
    fin = top > -np.inf
    safe = np.where(fin, top, 0.0)
    e = np.where(logw > -np.inf, np.exp(logw - safe[:, None]), 0.0)
    s = np.sum(e, axis=1)
    with np.errstate(divide="ignore"):
        lnz = np.where(fin, safe + np.log(np.where(fin, s, 1.0)), -np.inf)
    a = np.sum(np.where(e > 0, e * ll, 0.0), axis=1) if ll is not None else None
    return lnz, a, s


def _definition(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode, return_logwt):
    R = run_start.shape[0] - 1
    logz, info = np.empty((R, nsamples)), np.empty((R, nsamples))
    out_w = []
    for r in range(R):
        ll = logl[run_start[r]:run_start[r + 1]]
        w = np.empty((nsamples, ll.shape[0])) if return_logwt else None
        logz[r], info[r] = _one_run(ll, int(n_dead[r]), int(nlive[r]), int(kbatch[r]), int(seeds[r]), nsamples, mode == 1, w)
        out_w.append(w)
    return logz, info, out_w


def _device(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode, return_logwt, device, block_bytes, timing):
    lib = _abi.load()
    R = run_start.shape[0] - 1
    logz, info = np.empty((R, nsamples)), np.empty((R, nsamples))
    flat = np.empty(nsamples * logl.shape[0]) if return_logwt else None
    t = _abi.ShrinkTiming()
    _abi.check(lib.rvll_shrinkage_replicates(
        int(device), _abi.as_dp(logl), logl.shape[0], run_start.ctypes.data_as(C.POINTER(C.c_int64)), R,
        n_dead.ctypes.data_as(C.POINTER(C.c_int64)), _abi.as_ip(nlive), _abi.as_ip(kbatch),
        seeds.ctypes.data_as(C.POINTER(C.c_uint64)), nsamples, mode, _abi.as_dp(logz), _abi.as_dp(info),
        _abi.as_dp(flat) if flat is not None else None, int(block_bytes or 0), C.byref(t)))
    if timing is not None:
        timing.update(kernel_ms=t.kernel_ms, total_ms=t.total_ms, elements=t.elements, launches=t.launches,
                      threads=t.threads)
    out_w = [None] * R
    if flat is not None:
        for r in range(R):
            n = int(run_start[r + 1] - run_start[r])
            out_w[r] = flat[nsamples * run_start[r]:nsamples * run_start[r + 1]].reshape(nsamples, n)
    return logz, info, out_w


def replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples=1000, mode="random", return_logwt=False,
                      device=None, block_bytes=None, timing=None):
    """Replicates of R runs given as arrays: the rows run_start[r] .. run_start[r + 1] of logl are run r's dead rows in
    death order (n_dead[r] of them), then its final live rows.  Returns (logz [R, S], information [R, S]) and, with
    return_logwt, a list of R arrays logwt[r] [S, rows of run r] as a third element.  device=None evaluates the numpy
    definition; device=k runs rvll_shrinkage_replicates on device k (block_bytes: bound on the device memory the weights
    may take, default 512 MiB; timing: a dict that receives the call's rvll_shrink_timing)."""
    args = check_args(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode)
    if device is None:
        logz, info, w = _definition(*args, return_logwt)
    else:
        logz, info, w = _device(*args, return_logwt, device, block_bytes, timing)
    return (logz, info, w) if return_logwt else (logz, info)


def _schedule(res, nlive, kbatch):
    nl = res.nlive if getattr(res, "nlive", None) is not None else nlive
    kb = res.kbatch if getattr(res, "kbatch", None) is not None else kbatch
    if nl is None or kb is None:
        raise ValueError("a result without nlive / kbatch (made before they were recorded) needs nlive= and kbatch=")
    return int(nl), int(kb)


def replicates(results, nsamples=1000, seed=0, device=None, mode="random", return_logwt=False, nlive=None, kbatch=None,
               block_bytes=None, timing=None):
    """Simulated-shrinkage replicates of finished runs (a list of NestedResult): (logz [R, S], information [R, S]), and with
    return_logwt the ragged weights (a list of R arrays [S, len(result.logl)]).  Each result's nlive and kbatch come from
    the result; nlive= / kbatch= stand in for results that lack them.  seed: an int (run r then gets the splitmix64 word
    keep_words(seed, R)[r]) or one seed per run.  mode="expected" replaces the random shrinkage by its mean, and gives every
    run's own logz / information / logwt back.  device=None: the numpy definition; device=k: the GPU (rvll_shrinkage_replicates)."""
    results = list(results)
    R = len(results)
    seeds = keep_words(seed, R) if np.ndim(seed) == 0 else seed
    sched = [_schedule(res, nlive, kbatch) for res in results]
    logl = np.concatenate([np.asarray(res.logl, dtype=np.float64).reshape(-1) for res in results]) if R else np.zeros(0)
    run_start = np.concatenate([[0], np.cumsum([len(res.logl) for res in results])]).astype(np.int64)
    return replicates_arrays(logl, run_start, [res.niter for res in results], [s[0] for s in sched], [s[1] for s in sched],
                             seeds, nsamples, mode, return_logwt, device, block_bytes, timing)


def logz_error(results, nsamples=1000, seed=0, device=None, **kw):
    """float64 [R]: the standard deviation of ln Z over each run's simulated-shrinkage replicates."""
    return np.std(replicates(results, nsamples, seed, device, **kw)[0], axis=1)
