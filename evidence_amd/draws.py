"""Equal-weight posterior draws of merged nested-sampling runs: what dynesty's resample_equal, UltraNest's results['samples'] and
anesthetic's posterior_points give for one run, for every replicate of the merged run (merge.py: simulated shrinkage, optionally on
top of a bootstrap of the runs), so that anything computed from the draws — a curve band, m sin i with its own stellar-mass draws
— carries the run-to-run scatter.  The numpy definition below is the reference that the device entry
(rvll_draw_replicates; csrc/rvll_draws.hip) reproduces; on the device the replicated weights never cross to the host.

Replicate s is that of merge.replicates_arrays: the same seed_s, multiplicities and merged order.  With n = ndraws:

    p_i      exp(logwt_i), 0 for a row without weight
    m_i      rint(p_i 2^62) as int64: marginals.py's integer
    C_i      the inclusive running sum of m in merged order, an exact integer sum; M = C_{N-1} < 2^63
    U        the 53-bit integer behind uniform01(seed_s ^ DRAW_XOR, 0), which is U 2^-53
    Q, O     Q = M // n,  O = (U Q) >> 53 (a 116-bit product: Python integers here, two 64-bit words on the device)
    tau_k    k Q + O, k = 0 .. n - 1
    draw k   the first merged row i with C_i > tau_k: searchsorted(C, tau, "right")

This is systematic resampling with one uniform a replicate: row i is drawn floor(n p_i) or ceil(n p_i) times (p_i = m_i / M
exactly; the last M - n Q < n units of 2^-62 are never reached), a row with m_i = 0 is never drawn, and the draws of a replicate
ascend in merged order.  A replicate with M < n is a bootstrap of empty runs and all its draws are -1.  rows[s, k] holds the
*input* row (order[i]), so samples_stacked[rows] works directly.  Every decision is an integer comparison: the result does not
depend on batching, on block_bytes or on the other replicates.
"""
import ctypes as C

import numpy as np

from . import _abi, merge
from .shrinkage import replicate_seeds

DRAW_XOR = 0xA0761D6478BD642F        # the uniform of replicate s uses the seed seed_s ^ DRAW_XOR
MAX_DRAWS = 2 ** 20
SCALE = 2.0 ** 62
_BLOCK_ELEMS = 1 << 21               # (replicate, row) elements the numpy definition holds at a time, per array
_M64 = 2 ** 64 - 1
_i64p = C.POINTER(C.c_int64)


def uniform53(seed, counter=0):
    """The 53-bit integer U behind uniform01(seed, counter) of rvll_math.h, as a Python int: uniform01 returns U 2^-53."""
    z = (int(seed) + 0x9E3779B97F4A7C15 * (int(counter) + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return z >> 11


def fixed_point(logwt):
    """int64: m = rint(exp(logwt) 2^62), 0 for a row without weight (-inf, or the NaN of a replicate without any weight)."""
    with np.errstate(invalid="ignore"):
        p = np.exp(np.asarray(logwt, dtype=np.float64))
    return np.rint(np.where(p > 0.0, p, 0.0) * SCALE).astype(np.int64)


def thresholds(M, seed_s, ndraws):
    """int64 [ndraws]: tau_k = k Q + O of the replicate with the seed seed_s and the total M >= ndraws."""
    Q = int(M) // int(ndraws)
    O = (uniform53(int(seed_s) ^ DRAW_XOR) * Q) >> 53
    return O + Q * np.arange(int(ndraws), dtype=np.int64)


def pick(m, seed_s, ndraws):
    """int64 [ndraws]: the merged rows drawn from the integers m [N] (merged order) of the replicate with the seed seed_s; -1
    throughout when sum m < ndraws."""
    C_ = np.cumsum(np.asarray(m, dtype=np.int64), dtype=np.int64)
    M = int(C_[-1])
    if M < int(ndraws):
        return np.full(int(ndraws), -1, np.int64)
    return np.searchsorted(C_, thresholds(M, seed_s, ndraws), side="right").astype(np.int64)


def check_ndraws(ndraws):
    if int(ndraws) != ndraws or not 1 <= int(ndraws) <= MAX_DRAWS:
        raise ValueError(f"ndraws must be in [1, {MAX_DRAWS}]")
    return int(ndraws)


def _definition(logl, birth, run_start, ndraws, nsamples, code, bootstrap, seed):
    lay = merge._layout(logl, birth, run_start)
    N, R = logl.shape[0], lay["R"]
    order = lay["order"].astype(np.int64)
    seeds = replicate_seeds(seed, nsamples)
    logz, info = np.empty(nsamples), np.empty(nsamples)
    rows = np.empty((nsamples, ndraws), np.int64)
    step = max(1, _BLOCK_ELEMS // N)
    for s0 in range(0, nsamples, step):
        s1 = min(nsamples, s0 + step)
        w = merge.bootstrap_weights(seeds[s0:s1], R) if bootstrap else np.ones((s1 - s0, R), np.int64)
        logz[s0:s1], info[s0:s1], logw, _ = merge._block(lay, w, seeds[s0:s1], code == _abi.SHRINK_EXPECTED)
        for s in range(s0, s1):
            with np.errstate(invalid="ignore"):
                i = pick(fixed_point(logw[s - s0] - logz[s]), seeds[s], ndraws)
            rows[s] = np.where(i >= 0, order[np.maximum(i, 0)], -1)
    return rows, logz, info


def _device(logl, birth, run_start, ndraws, nsamples, code, bootstrap, seed, device, block_bytes, timing, fixed=None, msum=None):
    lib = _abi.load()
    N, R = logl.shape[0], run_start.shape[0] - 1
    logz, info = np.empty(nsamples), np.empty(nsamples)
    rows = np.empty((nsamples, ndraws), np.int32)
    t = _abi.DrawTiming()
    _abi.check(lib.rvll_draw_replicates(
        int(device), _abi.as_dp(logl), _abi.as_dp(birth), N, run_start.ctypes.data_as(_i64p), R, ndraws, nsamples, code,
        1 if bootstrap else 0, int(seed) & _M64, _abi.as_ip(rows), _abi.as_dp(logz), _abi.as_dp(info),
        fixed.ctypes.data_as(_i64p) if fixed is not None else None, msum.ctypes.data_as(_i64p) if msum is not None else None,
        int(block_bytes or 0), C.byref(t)))
    if timing is not None:
        timing.update({name: getattr(t, name) for name, _ in t._fields_})
    return rows.astype(np.int64), logz, info


def draw_arrays(logl, birth, run_start, ndraws, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, block_bytes=None,
                timing=None):
    """ndraws equal-weight draws from each of nsamples replicates of the merged run of the runs (logl, birth, run_start) as
    merge.replicates_arrays takes them: (rows int64 [S, ndraws], logz [S], information [S]).  rows holds input rows, ascending in
    merged order within a replicate, -1 throughout a replicate without weight (ln Z = -inf).  Replicate 0 with mode="expected",
    bootstrap=False is the plain equal-weight posterior sample of the merged run.  device=None evaluates the numpy definition;
    device=k runs rvll_draw_replicates on device k (block_bytes bounds the device block of weights, 8 N bytes a replicate;
    default 8 GiB, of which no more than nsamples replicates are allocated; timing: a dict that receives the call's
    rvll_draw_timing)."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    ndraws = check_ndraws(ndraws)
    if device is None:
        return _definition(logl, birth, run_start, ndraws, nsamples, code, bootstrap, seed)
    return _device(logl, birth, run_start, ndraws, nsamples, code, bootstrap, seed, device, block_bytes, timing)


def device_integers(logl, birth, run_start, ndraws, nsamples=1000, seed=0, mode="random", bootstrap=True, device=0, block_bytes=None):
    """The device call with its two optional outputs, for tests that hold the device to its own integers: (rows, logz,
    information, fixed int64 [S, N] — the m of every replicate in merged order — and msum int64 [S])."""
    logl, birth, run_start, nsamples, code = merge.check_args(logl, birth, run_start, nsamples, mode, bootstrap)
    ndraws = check_ndraws(ndraws)
    fixed, msum = np.empty((nsamples, logl.shape[0]), np.int64), np.empty(nsamples, np.int64)
    return _device(logl, birth, run_start, ndraws, nsamples, code, bootstrap, seed, device, block_bytes, None, fixed, msum) + (
        fixed, msum)


def draw(results, ndraws, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, block_bytes=None, timing=None):
    """draw_arrays for finished runs (a list of NestedResult with logl_birth): rows index the runs' rows stacked in the order of
    the list, as merge.merge stacks them."""
    _, logl, birth, run_start = merge._stack(results)
    return draw_arrays(logl, birth, run_start, ndraws, nsamples, seed, mode, bootstrap, device, block_bytes, timing)


def samples(results, ndraws, nsamples=1000, seed=0, mode="random", bootstrap=True, device=None, block_bytes=None, timing=None):
    """theta float64 [S, ndraws, ndim]: the parameter vectors of the draws of every replicate (NaN throughout a replicate
    without weight).  With nsamples=1, mode="expected", bootstrap=False: theta[0] is the equal-weight posterior sample of the
    merged run."""
    results, logl, birth, run_start = merge._stack(results)
    for i, res in enumerate(results):
        if getattr(res, "samples", None) is None or len(res.samples) != len(res.logl):
            raise ValueError(f"result {i} has no samples for its rows")
    stacked = np.concatenate([np.asarray(res.samples, dtype=np.float64).reshape(len(res.logl), -1) for res in results])
    rows, _, _ = draw_arrays(logl, birth, run_start, ndraws, nsamples, seed, mode, bootstrap, device, block_bytes, timing)
    theta = stacked[np.maximum(rows, 0)]
    theta[rows < 0] = np.nan
    return theta
