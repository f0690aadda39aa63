"""GpuRVModel — the host-side mirror of the reference's RVModel for the hot path.

Duck-types what the reference's sampler wrappers use from a model
(evidence/polychord/__init__.py:92,100-102,216-218; evidence/ultranest/__init__.py:93):
`.parnames` (sorted), `.log_likelihood(x)`, `.datadict`, `.fixedpardict`, `.nplanets`,
plus the batched forms the GPU exists for.  Every evaluation goes through the C-ABI
(include/rvll.h) into the HIP kernels; there is no host implementation.
"""
import ctypes as C
import threading
import weakref
from contextlib import contextmanager
from typing import Dict, Optional, Sequence

import numpy as np

from . import _abi
from .data import EpochTable
from .layout import compile_layout
from .priors import PriorSpec
from .stepout import PROPOSALS, check_proposal


# ---- large result arrays ---------------------------------------------------------------------------------
# A float64 array above glibc's 32 MB mmap threshold is a fresh mapping every time it is made and an munmap when it dies:
# 2.7 ms of page faults for the 40 MB of theta rows a 262144-point call returns — more than the call itself (1.8 ms;
# profiles/r03_stream_probe.txt).  Results of that size are therefore handed out from a small store of blocks that come back
# when the LAST array looking at them (the result or any view of it) is collected: the array's base is a lease object, numpy
# keeps it alive exactly as long as the memory is referenced, and its finalizer returns the block.
_RESULT_MIN_BYTES = 32 << 20
_RESULT_KEEP = 4                      # blocks kept for reuse (of any size); more are simply freed
_result_blocks = []                   # uint8 arrays
_result_lock = threading.RLock()      # (re-entrant: a lease's finalizer may run inside _result_array, at any allocation)


class _Lease:
    __slots__ = ("__array_interface__", "__weakref__")

    def __init__(self, block, shape):
        iface = dict(block.__array_interface__)
        iface.update(shape=tuple(shape), typestr="<f8", descr=[("", "<f8")], strides=None)
        self.__array_interface__ = iface


def _give_back(block):
    with _result_lock:
        if len(_result_blocks) < _RESULT_KEEP:
            _result_blocks.append(block)


def _result_array(shape):
    """An uninitialised C-contiguous float64 array of `shape` (np.empty below 32 MB)."""
    nbytes = 8 * int(np.prod(shape))
    if nbytes < _RESULT_MIN_BYTES:
        return np.empty(shape, dtype=np.float64)
    block = None
    with _result_lock:
        for i, b in enumerate(_result_blocks):
            if b.nbytes == nbytes:
                block = _result_blocks.pop(i)
                break
        if block is None and len(_result_blocks) >= _RESULT_KEEP:
            _result_blocks.pop(0)     # make room: the oldest block of another size goes
    if block is None:
        block = np.empty(nbytes, dtype=np.uint8)
    lease = _Lease(block, shape)
    weakref.finalize(lease, _give_back, block)
    return np.asarray(lease)


class GpuRVModel:
    """RV model with its epoch table resident on one MI355X.

    Parameters follow RVModel.__init__ (evidence/rvmodel/__init__.py:94-154):
    fixedpardict  {name: value} of fixed parameters
    datadict      {instrument: {'data': table with rjd|jdb, vrad, svrad}}  (or an EpochTable)
    parnames      names of the free parameters; theta is ordered as sorted(parnames)
    linpar_dict   optional {key: series[Ne]} for `linpar_{key}` terms (rvmodel:131-136,210-212)
    priordict     optional {parname: PriorSpec}; enables prior_transform*
    device        HIP device index (default: current device)
    tol, itmax    Newton stop rule of the Kepler solver; defaults 1e-4 and 10000 are what the
                  reference passes (rvmodel/__init__.py:466,491) — change them and parity is gone
    precision     "fp64" (the reference's arithmetic; the only parity mode), "mixed" (fp64 phase and
                  chi^2, fp32 Newton iteration) or "fp32" — BASELINE.json configs[4] tolerance sweep
    """

    def __init__(self, fixedpardict: Dict[str, float], datadict, parnames: Sequence[str],
                 linpar_dict: Optional[Dict[str, np.ndarray]] = None,
                 priordict: Optional[Dict[str, PriorSpec]] = None, device: int = -1,
                 tol: Optional[float] = None, itmax: Optional[int] = None, precision: str = "fp64"):
        self._lib = _abi.load()          # raises RvllLibraryError when the HIP library is absent
        self._h = _abi.Handle()
        self.fixedpardict = dict(fixedpardict)
        self.table = datadict if isinstance(datadict, EpochTable) else EpochTable.from_datadict(datadict)
        self.datadict = datadict if not isinstance(datadict, EpochTable) else self.table.to_datadict()
        self.insts = list(self.table.insts)
        self.linpar_dict = dict(linpar_dict) if linpar_dict else {}
        self.layout = compile_layout(parnames, self.fixedpardict, self.insts, list(self.linpar_dict))
        if tol is not None:
            self.layout.tol = float(tol)
        if itmax is not None:
            self.layout.itmax = int(itmax)
        if precision not in _abi.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_abi.PRECISIONS)}")
        self.precision = precision
        self.layout.precision = _abi.PRECISIONS[precision]
        self.parnames = list(self.layout.parnames)
        self.nplanets = self.layout.nplanets
        self.drift_in_model = self.layout.has_drift
        self.linpar_in_model = self.layout.has_linpar
        self.jitter_in_model = self.layout.has_jitter
        self.time, self.vrad, self.svrad = self.table.time, self.table.vrad, self.table.svrad
        self.model_path = None

        series = None
        if self.layout.linpar_names:
            series = np.ascontiguousarray(
                np.stack([np.asarray(self.linpar_dict[k], dtype=np.float64) for k in self.layout.linpar_names]))
            if series.shape != (len(self.layout.linpar_names), self.table.n_epochs):
                raise ValueError("each linpar series must have one value per epoch")
        self._series = series
        layout_c, self._layout_keep = self.layout.to_c()
        _abi.check(self._lib.rvll_create(
            C.byref(layout_c), _abi.as_dp(self.table.time), _abi.as_dp(self.table.vrad),
            _abi.as_dp(self.table.svrad), _abi.as_ip(self.table.inst_id), self.table.n_epochs,
            _abi.as_dp(series) if series is not None else None, int(device), C.byref(self._h)))
        # persistent buffers (and their ctypes pointers) of the scalar callbacks: per call only the copy of x
        # and one foreign call remain on the Python side
        nd = max(1, self.ndim)
        self._s_in, self._s_th = np.empty((1, nd)), np.empty((1, nd))
        self._s_out, self._s_flag = np.empty(1), np.zeros(1, dtype=np.int32)
        self._s_in_p, self._s_th_p = _abi.as_dp(self._s_in), _abi.as_dp(self._s_th)
        self._s_out_p, self._s_flag_p = _abi.as_dp(self._s_out), _abi.as_ip(self._s_flag)
        self.priordict = None
        self._device = int(device)             # as given: negative is the device that is current at a call
        self._live_n = 0                     # rows of the resident live set (live_init)
        self._runs = None                      # (R, n) of the resident ensemble (live_runs_init)
        if priordict is not None:
            self.set_priors(priordict)

    # ---- lifetime ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.rvll_destroy(self._h)
            self._h = _abi.Handle()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def ndim(self):
        return len(self.parnames)

    # ---- priors -------------------------------------------------------------------------
    def set_priors(self, priordict: Dict[str, PriorSpec]):
        """priordict[name] for every free parameter (evidence/polychord/__init__.py:152)."""
        specs = []
        for name in self.parnames:
            if name not in priordict:
                raise KeyError(name)
            specs.append(priordict[name])
        arr = (_abi.Prior * max(1, len(specs)))()
        for i, s in enumerate(specs):
            arr[i] = s.to_c()
        _abi.check(self._lib.rvll_set_priors(self._h, arr, len(specs)))
        self.priordict = dict(priordict)

    # ---- log-likelihood --------------------------------------------------------------------
    def _theta2d(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.ndim:
            raise ValueError(f"expected an array of shape (n, {self.ndim}), got {x.shape}")
        return x

    @staticmethod
    def _out_array(a, shape, name):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable
                and a.shape == tuple(shape)):
            raise ValueError(f"{name}: expected a writeable C-contiguous float64 array of shape {tuple(shape)}")
        return a

    def log_likelihood_batch(self, X, return_flags=False):
        """log-L of every row of X[n, ndim] -> float64[n] (one fused kernel launch)."""
        X = self._theta2d(X)
        n = X.shape[0]
        out = np.empty(n, dtype=np.float64)
        flags = np.zeros(n, dtype=np.int32)
        _abi.check(self._lib.rvll_loglike_batch(self._h, _abi.as_dp(X), n, _abi.as_dp(out), _abi.as_ip(flags)))
        return (out, flags) if return_flags else out

    def log_likelihood(self, x):
        """Scalar form, same signature as RVModel.log_likelihood (rvmodel/__init__.py:157)."""
        x = np.asarray(x, dtype=np.float64)
        if x.size != self.ndim:
            raise ValueError(f"expected {self.ndim} parameters, got {x.size}")
        self._s_in[0, :self.ndim] = x.ravel()
        rc = self._lib.rvll_loglike_batch(self._h, self._s_in_p, 1, self._s_out_p, self._s_flag_p)
        if rc:
            _abi.check(rc)
        return float(self._s_out[0])

    # ---- Keplerian curves for post-processing -----------------------------------------------------
    def _curves(self, X, time, mask):
        X = self._theta2d(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        time = np.ascontiguousarray(np.atleast_1d(time), dtype=np.float64)
        out = np.empty((X.shape[0], time.shape[0]), dtype=np.float64)
        _abi.check(self._lib.rvll_kep_rv_batch(self._h, _abi.as_dp(X), X.shape[0], _abi.as_dp(time), time.shape[0],
                                               int(mask), _abi.as_dp(out)))
        return out

    def kep_rv_batch(self, X, time, exclude_planet=None):
        """RVModel.kep_rv for every row of X: the summed Keplerian RV of all planets except
        `exclude_planet` (1-based, as rvmodel/__init__.py:343-385) at `time` -> [n, len(time)]."""
        if not (exclude_planet is None or type(exclude_planet) is int):
            raise AssertionError(f"exclude_planet has to be an {int}, got {type(exclude_planet)}.")   # rvmodel:365-366
        mask = (1 << self.nplanets) - 1
        if exclude_planet is not None and 1 <= exclude_planet <= self.nplanets:
            mask &= ~(1 << (exclude_planet - 1))
        return self._curves(X, time, mask)

    def modelk_batch(self, X, time, planet):
        """RVModel.modelk for every row of X: the Keplerian curve of one planet (1-based, rvmodel:388-463)."""
        if not 1 <= int(planet) <= self.nplanets:
            raise KeyError(f"planet{planet}_k1")
        return self._curves(X, time, 1 << (int(planet) - 1))

    def kep_rv_bands(self, theta, time, levels, planet=None, exclude_planet=None, chunk_bytes=None, timing=None):
        """Order statistics of groups of curves (predictive.bands_definition holds the definition; rvll_kep_rv_bands): theta
        [G, n, ndim] is G groups of n parameter vectors (n <= 4096), levels up to 16 numbers in (0, 1).  The curves are
        modelk_batch's for `planet`, else kep_rv_batch's with `exclude_planet`, bit for bit, and stay on the device.  Returns
        (q [G, len(levels), T], mean [G, T], n_valid int32 [G, T]): per group and time the quantiles by the inverted CDF of
        equal weights and the mean of the curves that are not NaN, and their number.  chunk_bytes bounds the device buffer of
        curve values (default 256 MiB, at least one group); the results do not depend on it.  timing: a dict that receives
        curves_ms and sort_ms."""
        from .predictive import check_levels
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[2] != self.ndim:
            raise ValueError(f"expected an array of shape (groups, n, {self.ndim}), got {theta.shape}")
        G, n = theta.shape[:2]
        if not 1 <= n <= 4096:
            raise ValueError("a group holds 1 to 4096 rows")
        levels = check_levels(levels)
        if planet is not None:
            if not 1 <= int(planet) <= self.nplanets:
                raise KeyError(f"planet{planet}_k1")
            mask = 1 << (int(planet) - 1)
        else:
            if not (exclude_planet is None or type(exclude_planet) is int):
                raise AssertionError(f"exclude_planet has to be an {int}, got {type(exclude_planet)}.")
            mask = (1 << self.nplanets) - 1
            if exclude_planet is not None and 1 <= exclude_planet <= self.nplanets:
                mask &= ~(1 << (exclude_planet - 1))
        time = np.ascontiguousarray(np.atleast_1d(time), dtype=np.float64)
        T, Q = time.shape[0], levels.shape[0]
        q, mean, nv = np.empty((G, Q, T)), np.empty((G, T)), np.empty((G, T), dtype=np.int32)
        ms = np.zeros(2)
        _abi.check(self._lib.rvll_kep_rv_bands(self._h, _abi.as_dp(theta), G, n, _abi.as_dp(time), T, int(mask), _abi.as_dp(levels),
                                               Q, _abi.as_dp(q), _abi.as_dp(mean), _abi.as_ip(nv), int(chunk_bytes or 0),
                                               _abi.as_dp(ms)))
        if timing is not None:
            timing.update(curves_ms=float(ms[0]), sort_ms=float(ms[1]))
        return q, mean, nv

    # ---- residuals of the likelihood's model and their periodograms (periodogram.py) -------------
    def _keep_mask(self, keep_planet):
        """The planets that are subtracted: all, or all but keep_planet (1-based; kep_rv_batch's exclude_planet semantics)."""
        if not (keep_planet is None or type(keep_planet) is int):
            raise AssertionError(f"keep_planet has to be an {int}, got {type(keep_planet)}.")
        mask = (1 << self.nplanets) - 1
        if keep_planet is not None and 1 <= keep_planet <= self.nplanets:
            mask &= ~(1 << (keep_planet - 1))
        return mask

    def residuals_batch(self, X, keep_planet=None):
        """`res` and `noise` of RVModel.log_likelihood (rvmodel/__init__.py:180-215) for every row of X -> (res [n, Ne], var
        [n, Ne]): the data minus the instruments' offsets, the Keplerian sum (kep_rv_batch(X, table.time, keep_planet), bit for
        bit), the drift and the linear terms; var = svrad² (+ jitter²).  keep_planet=p leaves planet p in the residuals.  An
        invalid orbit gives a NaN row of res.  periodogram.residuals_definition holds the definition."""
        X = self._theta2d(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        ne = self.table.time.shape[0]
        res, var = np.empty((X.shape[0], ne)), np.empty((X.shape[0], ne))
        _abi.check(self._lib.rvll_residuals_batch(self._h, _abi.as_dp(X), X.shape[0], int(self._keep_mask(keep_planet)),
                                                  _abi.as_dp(res), _abi.as_dp(var)))
        return res, var

    def gls_bands(self, theta, f0, df, nfreq, levels, keep_planet=None, return_power=False, chunk_bytes=None, timing=None):
        """Generalised Lomb-Scargle periodograms of the residuals of groups of parameter vectors and their order statistics
        (periodogram.gls_definition and predictive.bands_definition hold the definitions; rvll_gls_bands): theta [G, n, ndim]
        is G groups of n rows (n <= 4096), the grid f0 + df k for k < nfreq, levels up to 16 numbers in (0, 1).  Returns a dict:
        q [G, len(levels), F], mean [G, F], n_valid int32 [G, F] over every group's powers per frequency, peak_index int32
        [G, n] (the first index of a row's largest power; -1 for an invalid orbit), peak_power [G, n], and with return_power
        power [G, n, F].  chunk_bytes bounds the device buffers of a chunk of groups (default 256 MiB, at least one group); no
        result depends on it.  timing: a dict that receives residuals_ms, gls_ms and reduce_ms."""
        from .periodogram import check_grid
        from .predictive import check_levels
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[2] != self.ndim:
            raise ValueError(f"expected an array of shape (groups, n, {self.ndim}), got {theta.shape}")
        G, n = theta.shape[:2]
        if not 1 <= n <= 4096:
            raise ValueError("a group holds 1 to 4096 rows")
        levels = check_levels(levels)
        f0, df, F = check_grid(f0, df, nfreq, self.table.time.shape[0])
        mask = self._keep_mask(keep_planet)
        Q = levels.shape[0]
        q, mean, nv = np.empty((G, Q, F)), np.empty((G, F)), np.empty((G, F), dtype=np.int32)
        pidx, ppow = np.empty((G, n), dtype=np.int32), np.empty((G, n))
        power = np.empty((G, n, F)) if return_power else None
        ms = np.zeros(3)
        _abi.check(self._lib.rvll_gls_bands(self._h, _abi.as_dp(theta), G, n, int(mask), f0, df, F, _abi.as_dp(levels), Q,
                                            _abi.as_dp(q), _abi.as_dp(mean), _abi.as_ip(nv), _abi.as_ip(pidx), _abi.as_dp(ppow),
                                            _abi.as_dp(power) if return_power else None, int(chunk_bytes or 0), _abi.as_dp(ms)))
        if timing is not None:
            timing.update(residuals_ms=float(ms[0]), gls_ms=float(ms[1]), reduce_ms=float(ms[2]))
        out = dict(q=q, mean=mean, n_valid=nv, peak_index=pidx, peak_power=ppow)
        if return_power:
            out["power"] = power
        return out

    def gls_batch(self, X, f0, df, nfreq, keep_planet=None):
        """The periodogram of every row's residuals -> power [n, F]: gls_bands' powers, the rows sent as groups of up to 4096
        (a power's bits depend on its row and frequency alone)."""
        X = self._theta2d(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        out = []
        for lo in range(0, X.shape[0], 4096):
            part = X[lo:lo + 4096]
            out.append(self.gls_bands(part[None], f0, df, nfreq, [0.5], keep_planet=keep_planet, return_power=True)["power"][0])
        return np.concatenate(out, axis=0) if out else np.empty((0, int(nfreq)))

    # ---- prior transform --------------------------------------------------------------------
    def prior_transform_batch(self, cubes):
        cubes = self._theta2d(cubes)
        out = _result_array(cubes.shape)
        _abi.check(self._lib.rvll_prior_batch(self._h, _abi.as_dp(cubes), cubes.shape[0], _abi.as_dp(out)))
        return out

    def log_prior_batch(self, thetas):
        """ln pi(theta) [n] of the rows of thetas [n, ndim] under the model's own priors: the density of the transform
        prior_transform_batch applies, on the model's device (rvll_prior_logpdf_batch; priors.log_density is the numpy
        definition).  -inf outside the support.  Needs the priors (priordict=)."""
        if self.priordict is None:
            raise _abi.RvllError(_abi.E_NOPRIORS, "log_prior_batch needs the priors (priordict=)")
        from .sensitivity import log_prior_sets
        thetas = self._theta2d(thetas)
        return log_prior_sets([[self.priordict[name] for name in self.parnames]], thetas, device=self._device)[:, 0]

    def prior_transform(self, cube):
        cube = np.asarray(cube, dtype=np.float64)
        if cube.size != self.ndim:
            raise ValueError(f"expected {self.ndim} coordinates, got {cube.size}")
        self._s_in[0, :self.ndim] = cube.ravel()
        rc = self._lib.rvll_prior_batch(self._h, self._s_in_p, 1, self._s_th_p)
        if rc:
            _abi.check(rc)
        return self._s_th[0, :self.ndim].copy().reshape(cube.shape)

    def prior_loglike(self, cube):
        """Scalar pair: prior(cube) and the log-L of the result in ONE call — (theta, logL).  With the scalar server on,
        one request of the persistent kernel instead of two (what PolyChord's prior + loglike sequence amounts to)."""
        cube = np.asarray(cube, dtype=np.float64)
        if cube.size != self.ndim:
            raise ValueError(f"expected {self.ndim} coordinates, got {cube.size}")
        self._s_in[0, :self.ndim] = cube.ravel()
        rc = self._lib.rvll_prior_loglike_batch(self._h, self._s_in_p, 1, self._s_th_p, self._s_out_p, self._s_flag_p)
        if rc:
            _abi.check(rc)
        return self._s_th[0, :self.ndim].copy().reshape(cube.shape), float(self._s_out[0])

    def prior_loglike_batch(self, cubes, return_flags=False, theta_out=None, logl_out=None):
        """Fused prior(cube) -> theta -> log-L: one upload, two launches, one download.

        theta_out / logl_out: arrays to fill (C-contiguous float64, (n, ndim) and (n,)) — a caller that evaluates hundreds of
        thousands of rows per call keeps them between calls: above glibc's 32 MB mmap threshold a fresh result array is a
        fresh mapping, and its page faults cost more than the whole call (profiles/r03_stream_probe.txt)."""
        cubes = self._theta2d(cubes)
        n = cubes.shape[0]
        theta = _result_array((n, self.ndim)) if theta_out is None else self._out_array(theta_out, (n, self.ndim), "theta_out")
        out = np.empty(n, dtype=np.float64) if logl_out is None else self._out_array(logl_out, (n,), "logl_out")
        flags = np.zeros(n, dtype=np.int32)
        _abi.check(self._lib.rvll_prior_loglike_batch(self._h, _abi.as_dp(cubes), n, _abi.as_dp(theta),
                                                      _abi.as_dp(out), _abi.as_ip(flags)))
        return (theta, out, flags) if return_flags else (theta, out)

    # ---- device-resident forms (bench / multi-GPU) ----------------------------------------------
    def dev_reserve(self, n):
        _abi.check(self._lib.rvll_dev_reserve(self._h, int(n)))

    def dev_upload_theta(self, X):
        X = self._theta2d(X)
        _abi.check(self._lib.rvll_dev_upload_theta(self._h, _abi.as_dp(X), X.shape[0]))

    def dev_upload_cube(self, cubes):
        cubes = self._theta2d(cubes)
        _abi.check(self._lib.rvll_dev_upload_cube(self._h, _abi.as_dp(cubes), cubes.shape[0]))

    def dev_fill_cube(self, n, seed):
        _abi.check(self._lib.rvll_dev_fill_cube(self._h, int(n), int(seed)))

    def dev_prior(self, n):
        _abi.check(self._lib.rvll_dev_prior(self._h, int(n)))

    def dev_loglike(self, n):
        _abi.check(self._lib.rvll_dev_loglike(self._h, int(n)))

    def slice_walk(self, cube, theta, logl, lstar, chol, wrapped=None, nsteps=10, max_rounds=200, seed=0,
                   walker_base=0, proposal=None, step_width=None):
        """nsteps slice-sampling moves of every walker inside logL > lstar, entirely on the GPU
        (rvll_slice_walk).  cube/theta/logl are the walkers' start points; returns (cube, theta, logl, ncalls)
        of the end points.  chol: lower-triangular factor of the live points' covariance in the unit cube.
        walker_base: index of the first row in a larger set of walkers (sharded walks draw the same random numbers
        as the unsharded one)."""
        cube = np.array(self._theta2d(cube), dtype=np.float64, order="C")
        theta = np.array(self._theta2d(theta), dtype=np.float64, order="C")
        logl = np.array(logl, dtype=np.float64).reshape(-1)
        k = cube.shape[0]
        if theta.shape != cube.shape or logl.shape[0] != k:
            raise ValueError("cube, theta and logl must describe the same walkers")
        chol = np.ascontiguousarray(chol, dtype=np.float64)
        if chol.shape != (self.ndim, self.ndim):
            raise ValueError("chol must be [ndim, ndim]")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        ncalls = C.c_int64(0)
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_slice_walk(
                self._h, _abi.as_dp(cube), _abi.as_dp(theta), _abi.as_dp(logl), k, float(lstar), _abi.as_dp(chol),
                _abi.as_ip(wr) if wr is not None else None, int(nsteps), int(max_rounds), int(seed) & (2 ** 64 - 1),
                int(walker_base), C.byref(ncalls)))
        return cube, theta, logl, int(ncalls.value)

    def slice_walk_runs(self, cube, theta, logl, run_start, lstar, chol, wrapped=None, nsteps=10, max_rounds=200, seeds=(),
                        proposal=None, step_width=None):
        """The walks of R independent runs in ONE device walk (rvll_slice_walk_runs).  Rows run_start[r] .. run_start[r + 1]
        of cube / theta / logl are the walkers of run r, which walks inside logL > lstar[r] with the whitening factor
        chol[r] ([R, ndim, ndim]) and seed seeds[r].  Returns (cube, theta, logl, ncalls[R]); run r's rows and ncalls[r] are
        bit for bit those of slice_walk(its rows, lstar[r], chol[r], wrapped, nsteps, max_rounds, seeds[r]).  nsteps is an int
        (every run) or one count per run ([R]: rvll_slice_walk_runs_steps, run r then walks as slice_walk(..., nsteps[r], ...))."""
        cube = np.array(self._theta2d(cube), dtype=np.float64, order="C")
        theta = np.array(self._theta2d(theta), dtype=np.float64, order="C")
        logl = np.array(logl, dtype=np.float64).reshape(-1)
        k = cube.shape[0]
        if theta.shape != cube.shape or logl.shape[0] != k:
            raise ValueError("cube, theta and logl must describe the same walkers")
        run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
        nrun = run_start.shape[0] - 1
        if nrun < 0 or run_start[0] != 0 or run_start[-1] != k or np.any(np.diff(run_start) < 0):
            raise ValueError("run_start must rise from 0 to the number of walkers")
        lstar = np.ascontiguousarray(lstar, dtype=np.float64).reshape(-1)
        seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
        if lstar.shape[0] != nrun or seeds.shape[0] != nrun:
            raise ValueError("lstar and seeds need one entry per run")
        chol = np.ascontiguousarray(chol, dtype=np.float64)
        if chol.shape != (nrun, self.ndim, self.ndim):
            raise ValueError("chol must be [runs, ndim, ndim]")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        ncalls = np.zeros(nrun, dtype=np.int64)
        if np.ndim(nsteps) != 0:
            steps = np.ascontiguousarray(nsteps, dtype=np.int32).reshape(-1)
            if steps.shape[0] != nrun:
                raise ValueError("nsteps needs one entry per run (or one int for all)")
            with self._proposal_for(proposal, step_width):
                _abi.check(self._lib.rvll_slice_walk_runs_steps(
                    self._h, _abi.as_dp(cube), _abi.as_dp(theta), _abi.as_dp(logl),
                    run_start.ctypes.data_as(C.POINTER(C.c_int64)), nrun, _abi.as_dp(lstar), _abi.as_dp(chol),
                    seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _abi.as_ip(wr) if wr is not None else None,
                    _abi.as_ip(steps), int(max_rounds), ncalls.ctypes.data_as(C.POINTER(C.c_int64))))
            return cube, theta, logl, ncalls
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_slice_walk_runs(
                self._h, _abi.as_dp(cube), _abi.as_dp(theta), _abi.as_dp(logl),
                run_start.ctypes.data_as(C.POINTER(C.c_int64)), nrun, _abi.as_dp(lstar), _abi.as_dp(chol),
                seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _abi.as_ip(wr) if wr is not None else None,
                int(nsteps), int(max_rounds), ncalls.ctypes.data_as(C.POINTER(C.c_int64))))
        return cube, theta, logl, ncalls

    def walk_distances_runs(self, survivors, group_start, factors, wrapped, starts, ends, walker_group):
        """The distances of the step-count adaptation on the device (rvll_walk_distances_runs): rows
        group_start[g] .. group_start[g + 1] of survivors ([N, ndim] unit-cube rows) are group g, whitened by factors[g]
        ([G, ndim, ndim]); walker k went from starts[k] to ends[k] in group walker_group[k].  Returns (pair [G], move [K]) —
        adapt.walk_distances_runs's: move bit for bit, pair to round-off (its summation order)."""
        from .adapt import check_args
        survivors, group_start, factors, wrapped, starts, ends, walker_group = check_args(
            self._theta2d(survivors), group_start, factors, wrapped, starts, ends, walker_group)
        if survivors.shape[1] != self.ndim:
            raise ValueError("rows must have ndim columns")
        G, K = group_start.shape[0] - 1, starts.shape[0]
        wr = None if wrapped is None else np.ascontiguousarray(wrapped.astype(np.int32))
        pair = np.empty(G, dtype=np.float64)
        move = np.empty(K, dtype=np.float64)
        _abi.check(self._lib.rvll_walk_distances_runs(
            self._h, _abi.as_dp(survivors), group_start.ctypes.data_as(C.POINTER(C.c_int64)), G, _abi.as_dp(factors),
            _abi.as_ip(wr) if wr is not None else None, _abi.as_dp(starts), _abi.as_dp(ends), _abi.as_ip(walker_group), K,
            _abi.as_dp(pair), _abi.as_dp(move)))
        return pair, move

    def cluster_runs(self, cube, run_start, scale, wrapped=None, nboot=30, seeds=()):
        """MLFriends clustering of R independent row sets in one device call (rvll_cluster_runs).  Rows
        run_start[r] .. run_start[r + 1] of cube ([N, ndim] unit-cube rows) are run r, with metric scale[r] ([R, ndim]) and
        bootstrap seed seeds[r]; wrapped [ndim] marks circular dimensions.  Returns (labels [N] int32, nclusters [R] int32,
        radius2 [R] float64), bit for bit those of clustering.cluster_runs."""
        cube = np.ascontiguousarray(self._theta2d(cube), dtype=np.float64)
        run_start = np.ascontiguousarray(run_start, dtype=np.int64).reshape(-1)
        R = run_start.shape[0] - 1
        if R < 0:
            raise ValueError("run_start needs at least one entry")
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        if scale.size != R * self.ndim:
            raise ValueError("scale must be [runs, ndim]")
        seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
        if seeds.shape[0] != R:
            raise ValueError("seeds needs one entry per run")
        if R > 0 and run_start[-1] != cube.shape[0]:
            raise ValueError("run_start must end at the number of rows")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        labels = np.zeros(cube.shape[0], dtype=np.int32)
        nclusters = np.zeros(max(R, 0), dtype=np.int32)
        radius2 = np.zeros(max(R, 0), dtype=np.float64)
        _abi.check(self._lib.rvll_cluster_runs(
            self._h, _abi.as_dp(cube), run_start.ctypes.data_as(C.POINTER(C.c_int64)), R, _abi.as_dp(scale),
            _abi.as_ip(wr) if wr is not None else None, int(nboot), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
            _abi.as_ip(labels), _abi.as_ip(nclusters), _abi.as_dp(radius2)))
        return labels, nclusters, radius2

    def region_tile_rows(self):
        """The survivors of a run that one LDS image of the region sampler's neighbour count holds (more are tiled)."""
        rows = C.c_int32(0)
        _abi.check(self._lib.rvll_region_tile_rows(self.ndim, C.byref(rows)))
        return int(rows.value)

    def region_draw_runs(self, survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped=None, max_candidates=None,
                         trace=False, first=0, block=None, trace_cap=None, return_rounds=False):
        """MLFriends region sampling of R runs in one device call (rvll_region_draw_runs; region.draw_runs is the
        definition, with this model's prior transform and log-L as its `evaluate`).  Returns (cube [R, kdraw, ndim], theta
        [R, kdraw, ndim], logl [R, kdraw], nfound [R] int32, ncalls [R] int64), rows past nfound NaN.  trace=True adds a list
        of R dicts (c, cube, flags, n, logl) over the first trace_cap candidates every run evaluated (default: all of them);
        return_rounds=True adds the rounds the call took.  Needs the priors (priordict=)."""
        from . import region as _region
        if max_candidates is None:
            max_candidates = _region.DEFAULT_MAX_CANDIDATES
        if block is None:
            block = _region.DEFAULT_BLOCK
        survivors = np.ascontiguousarray(self._theta2d(survivors), dtype=np.float64)
        survivors, run_start, scale, radius2, lstar, seeds, kdraw, wr, first, max_candidates, block = _region.check_args(
            survivors, run_start, scale, radius2, lstar, seeds, kdraw, wrapped, first, max_candidates, block)
        R, D = run_start.shape[0] - 1, self.ndim
        wi = None if wr is None else np.ascontiguousarray(wr.astype(np.int32))
        cube = np.full((R, kdraw, D), np.nan)
        theta = np.full((R, kdraw, D), np.nan)
        logl = np.full((R, kdraw), np.nan)
        nfound = np.zeros(R, dtype=np.int32)
        ncalls = np.zeros(R, dtype=np.int64)
        cap = 0
        if trace:
            cap = int(max_candidates if trace_cap is None else trace_cap)
        tcube = np.full((R, cap, D), np.nan)
        tflags = np.zeros((R, cap), dtype=np.int32)
        tn = np.zeros((R, cap), dtype=np.int32)
        tlogl = np.full((R, cap), np.nan)
        tcount = np.zeros(R, dtype=np.int64)
        rounds = C.c_int32(0)
        i64 = C.POINTER(C.c_int64)
        _abi.check(self._lib.rvll_region_draw_runs(
            self._h, _abi.as_dp(survivors), run_start.ctypes.data_as(i64), R, _abi.as_dp(scale), _abi.as_dp(radius2),
            _abi.as_dp(lstar), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), _abi.as_ip(wi) if wi is not None else None,
            kdraw, first, max_candidates, block, _abi.as_dp(cube), _abi.as_dp(theta), _abi.as_dp(logl), _abi.as_ip(nfound),
            ncalls.ctypes.data_as(i64), cap, _abi.as_dp(tcube) if cap else None, _abi.as_ip(tflags) if cap else None,
            _abi.as_ip(tn) if cap else None, _abi.as_dp(tlogl) if cap else None, tcount.ctypes.data_as(i64) if cap else None,
            C.byref(rounds)))
        out = (cube, theta, logl, nfound, ncalls)
        if trace:
            out += ([{"c": np.arange(first, first + int(tcount[r]), dtype=np.uint64), "cube": tcube[r, :tcount[r]].copy(),
                      "flags": tflags[r, :tcount[r]].copy(), "n": tn[r, :tcount[r]].astype(np.int64),
                      "logl": tlogl[r, :tcount[r]].copy()} for r in range(R)],)
        if return_rounds:
            out += (int(rounds.value),)
        return out

    def cluster(self, cube, scale, wrapped=None, nboot=30, seed=0):
        """One run of cluster_runs: (labels [N], nclusters, radius2)."""
        cube = self._theta2d(cube)
        labels, nclusters, radius2 = self.cluster_runs(cube, [0, cube.shape[0]], np.reshape(scale, (1, -1)), wrapped,
                                                       nboot, [seed])
        return labels, int(nclusters[0]), float(radius2[0])

    # ---- live set resident on the device (nested.run_nested_slice(..., live=model)) -----------------------------
    def live_init(self, cube):
        """N unit-cube rows -> prior transform -> log-L; the live set stays on the device.  Returns log-L [N]."""
        cube = self._theta2d(cube)
        logl = np.empty(cube.shape[0], dtype=np.float64)
        self._runs = None
        _abi.check(self._lib.rvll_live_init(self._h, _abi.as_dp(cube), cube.shape[0], _abi.as_dp(logl)))
        self._live_n = cube.shape[0]
        return logl

    def live_step(self, order, kdead, start, lstar, wrapped=None, nsteps=10, max_rounds=200, seed=0, walker_base=0,
                  chol=None, return_chol=False, proposal=None, step_width=None):
        """One iteration of nested sampling on the resident live set (include/rvll.h, rvll_live_step): rows order[:kdead]
        die (kept in the device's dead store), kdead walkers start from rows `start`, walk, and replace them.  chol=None:
        the whitening comes from the surviving rows' covariance, computed on the device.  Returns (logl_new[kdead], ncalls)
        (+ the factor used with return_chol)."""
        order = None if order is None else np.ascontiguousarray(order, dtype=np.int32)     # None: the order live_sort left on the device
        start = np.ascontiguousarray(start, dtype=np.int32)
        kdead = int(kdead)
        if self._live_n < 1:
            raise RuntimeError("live_init has not been called")
        if (order is not None and order.shape != (self._live_n,)) or start.shape != (kdead,):
            raise ValueError("order must list every live row, start one row per dying point")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        ch = None if chol is None else np.ascontiguousarray(chol, dtype=np.float64)
        if ch is not None and ch.shape != (self.ndim, self.ndim):
            raise ValueError("chol must be [ndim, ndim]")
        logl_new = np.empty(kdead, dtype=np.float64)
        used = np.empty((self.ndim, self.ndim)) if return_chol else None
        ncalls = C.c_int64(0)
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_live_step(
                self._h, _abi.as_ip(order) if order is not None else None, kdead, _abi.as_ip(start), float(lstar), _abi.as_dp(ch) if ch is not None else None,
                _abi.as_ip(wr) if wr is not None else None, int(nsteps), int(max_rounds), int(seed) & (2 ** 64 - 1),
                int(walker_base), C.byref(ncalls), _abi.as_dp(logl_new), _abi.as_dp(used) if used is not None else None))
        return (logl_new, int(ncalls.value), used) if return_chol else (logl_new, int(ncalls.value))

    def live_sort(self, kdead):
        """Sort the resident live points by log-L ON THE DEVICE (include/rvll.h, rvll_live_sort): returns (log-L of the kdead
        lowest in ascending order, lstar = the kdead-th lowest, the highest log-L).  The live_step that follows is called with
        order=None and `start` as ranks among the survivors."""
        kdead = int(kdead)
        if self._live_n < 1:
            raise RuntimeError("live_init has not been called")
        dead = np.empty(kdead, dtype=np.float64)
        lstar, top = C.c_double(), C.c_double()
        _abi.check(self._lib.rvll_live_sort(self._h, kdead, _abi.as_dp(dead), C.byref(lstar), C.byref(top)))
        return dead, lstar.value, top.value

    def live_get(self, cube=True, theta=True, logl=True, theta_out=None):
        """(cube, theta, logl) of the resident live set (None for the ones switched off); theta_out: a C-contiguous
        [n, ndim] float64 array (or view) to receive theta in place."""
        n = self._live_n
        u = np.empty((n, self.ndim)) if cube else None
        th = (theta_out if theta_out is not None else np.empty((n, self.ndim))) if theta else None
        ll = np.empty(n) if logl else None
        if th is not None and (th.shape != (n, self.ndim) or th.dtype != np.float64 or not th.flags.c_contiguous):
            raise ValueError("theta_out must be a C-contiguous float64 array of shape (n, ndim)")
        _abi.check(self._lib.rvll_live_get(self._h, _abi.as_dp(u) if cube else None, _abi.as_dp(th) if theta else None,
                                           _abi.as_dp(ll) if logl else None))
        return u, th, ll

    def live_dead_count(self):
        n = C.c_int64(0)
        _abi.check(self._lib.rvll_live_dead(self._h, C.byref(n), None, None))
        return int(n.value)

    def live_dead(self, theta_out=None):
        """(theta, logl) of every point that died so far, in the order they died; theta_out: a C-contiguous
        [n_dead, ndim] float64 array (or view) to receive theta in place."""
        n = self.live_dead_count()
        th = theta_out if theta_out is not None else np.empty((n, self.ndim))
        if th.shape != (n, self.ndim) or th.dtype != np.float64 or not th.flags.c_contiguous:
            raise ValueError("theta_out must be a C-contiguous float64 array of shape (n_dead, ndim)")
        ll = np.empty(n)
        if n:
            cnt = C.c_int64(n)
            _abi.check(self._lib.rvll_live_dead(self._h, C.byref(cnt), _abi.as_dp(th), _abi.as_dp(ll)))
        return th, ll

    def live_births(self):
        """(dead, live): the birth contours (rvll_live_births) of every point that died so far, in the order they died, and of
        the live points as live_get orders them — -inf for a point of live_init, else the lstar of the step that drew it."""
        n = self.live_dead_count()
        dead, live = np.empty(n), np.empty(self._live_n)
        cnt = C.c_int64(n)
        _abi.check(self._lib.rvll_live_births(self._h, C.byref(cnt), _abi.as_dp(dead), _abi.as_dp(live)))
        return dead, live

    # ---- the resident ensemble: R live sets in one handle (nested.run_nested_ensemble(..., live=model)) -----------------
    def live_runs_init(self, cube, nruns):
        """R = nruns independent live sets of n rows each (cube [R n, ndim]; run r = rows r n .. r n + n - 1) -> prior
        transform -> log-L, resident on the device (rvll_live_runs_init).  Replaces any resident live set.  Returns log-L [R, n]."""
        cube = np.ascontiguousarray(self._theta2d(cube), dtype=np.float64)
        nruns = int(nruns)
        if nruns < 1 or cube.shape[0] % nruns:
            raise ValueError("cube must hold nruns live sets of equally many rows")
        n = cube.shape[0] // nruns
        logl = np.empty((nruns, n), dtype=np.float64)
        self._live_n = 0
        _abi.check(self._lib.rvll_live_runs_init(self._h, _abi.as_dp(cube), nruns, n, _abi.as_dp(logl)))
        self._runs = (nruns, n)
        return logl

    def _runs_list(self, runs):
        if getattr(self, "_runs", None) is None:
            raise RuntimeError("live_runs_init has not been called")
        runs = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1)
        if runs.size < 1:
            raise ValueError("need at least one run")
        return runs

    def live_runs_sort(self, runs, kdead):
        """Sort every listed run's live points by log-L ON THE DEVICE (rvll_live_runs_sort): returns (log-L of each run's kdead
        lowest in ascending order [A, kdead], lstar [A], the highest log-L [A])."""
        runs = self._runs_list(runs)
        kdead = int(kdead)
        dead = np.empty((runs.size, kdead), dtype=np.float64)
        lstar, top = np.empty(runs.size), np.empty(runs.size)
        _abi.check(self._lib.rvll_live_runs_sort(self._h, _abi.as_ip(runs), runs.size, kdead, _abi.as_dp(dead), _abi.as_dp(lstar),
                                                 _abi.as_dp(top)))
        return dead, lstar, top

    def _live_runs_step_steps(self, runs, kdead, ranks, lstar, wr, nsteps, max_rounds, seeds, clustered, nboot, boot_seeds,
                              return_distances, proposal=None, step_width=None):
        """rvll_live_runs_step_steps (the arguments checked by the caller): (logl_new, ncalls, nclusters or None, move, pair)."""
        A = runs.size
        steps = np.ascontiguousarray(np.broadcast_to(np.asarray(nsteps, dtype=np.int32), (A,)))
        logl_new = np.empty((A, kdead), dtype=np.float64)
        ncalls = np.zeros(A, dtype=np.int64)
        nclusters = np.zeros(A, dtype=np.int32) if clustered else None
        move = np.empty((A, kdead), dtype=np.float64) if return_distances else None
        pair = np.empty((A, kdead), dtype=np.float64) if return_distances else None
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_live_runs_step_steps(
                self._h, _abi.as_ip(runs), A, kdead, _abi.as_ip(ranks), _abi.as_dp(lstar), _abi.as_ip(wr) if wr is not None else None,
                _abi.as_ip(steps), int(max_rounds), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), 1 if clustered else 0, int(nboot),
                boot_seeds.ctypes.data_as(C.POINTER(C.c_uint64)) if clustered else None, ncalls.ctypes.data_as(C.POINTER(C.c_int64)),
                _abi.as_dp(logl_new), _abi.as_ip(nclusters) if clustered else None, _abi.as_dp(move) if return_distances else None,
                _abi.as_dp(pair) if return_distances else None))
        return logl_new, ncalls, nclusters, move, pair

    def live_runs_step(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=(), return_chol=False,
                       return_distances=False, proposal=None, step_width=None):
        """One iteration of every listed run on the resident ensemble (rvll_live_runs_step), after live_runs_sort of the same
        runs: ranks [A, kdead] among each run's survivors, lstar [A] as live_runs_sort returned them, seeds [A].  Returns
        (logl_new [A, kdead], ncalls [A]) (+ the whitening factors [A, ndim, ndim] with return_chol); run a's part is bit for
        bit what live_step(None, kdead, ranks[a], lstar[a], ..., seeds[a]) gives a model that holds only that run.
        nsteps may be one count per run ([A]), and return_distances=True appends (move, pair) [A, kdead], the step-count
        adaptation's distances (rvll_live_runs_step_steps); neither goes with return_chol."""
        runs = self._runs_list(runs)
        kdead = int(kdead)
        A = runs.size
        ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        lstar = np.ascontiguousarray(lstar, dtype=np.float64).reshape(-1)
        seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
        if ranks.shape != (A, kdead):
            raise ValueError("ranks must be [runs, kdead]")
        if lstar.shape != (A,) or seeds.shape != (A,):
            raise ValueError("lstar and seeds need one entry per run")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        if np.ndim(nsteps) != 0 or return_distances:
            if return_chol:
                raise ValueError("return_chol does not go with a step table or return_distances")
            if np.ndim(nsteps) != 0 and np.shape(nsteps) != (A,):
                raise ValueError("nsteps needs one entry per run (or one int for all)")
            logl_new, ncalls, _, move, pair = self._live_runs_step_steps(runs, kdead, ranks, lstar, wr, nsteps, max_rounds, seeds,
                                                                         False, 0, None, return_distances, proposal, step_width)
            return (logl_new, ncalls, move, pair) if return_distances else (logl_new, ncalls)
        logl_new = np.empty((A, kdead), dtype=np.float64)
        ncalls = np.zeros(A, dtype=np.int64)
        used = np.empty((A, self.ndim, self.ndim)) if return_chol else None
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_live_runs_step(
                self._h, _abi.as_ip(runs), A, kdead, _abi.as_ip(ranks), _abi.as_dp(lstar), _abi.as_ip(wr) if wr is not None else None,
                int(nsteps), int(max_rounds), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), ncalls.ctypes.data_as(C.POINTER(C.c_int64)),
                _abi.as_dp(logl_new), _abi.as_dp(used) if used is not None else None))
        return (logl_new, ncalls, used) if return_chol else (logl_new, ncalls)

    def live_runs_step_clustered(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=(), nboot=30,
                                 boot_seeds=(), return_distances=False, proposal=None, step_width=None):
        """live_runs_step with the survivors of every listed run clustered on the device (rvll_live_runs_step_clustered; DESIGN
        §4e): run a's walkers are grouped by the cluster of their start row and whitened by that cluster's covariance, the
        clustering bootstrapped with boot_seeds[a].  Returns (logl_new [A, kdead] in walker order, ncalls [A], nclusters [A]).
        nsteps may be one count per run ([A]); return_distances=True appends (move, pair) [A, kdead] (rvll_live_runs_step_steps)."""
        runs = self._runs_list(runs)
        kdead = int(kdead)
        A = runs.size
        ranks = np.ascontiguousarray(ranks, dtype=np.int32)
        lstar = np.ascontiguousarray(lstar, dtype=np.float64).reshape(-1)
        seeds = np.array([int(s) & (2 ** 64 - 1) for s in seeds], dtype=np.uint64)
        boot_seeds = np.array([int(s) & (2 ** 64 - 1) for s in boot_seeds], dtype=np.uint64)
        if ranks.shape != (A, kdead):
            raise ValueError("ranks must be [runs, kdead]")
        if lstar.shape != (A,) or seeds.shape != (A,) or boot_seeds.shape != (A,):
            raise ValueError("lstar, seeds and boot_seeds need one entry per run")
        wr = None if wrapped is None else np.ascontiguousarray(np.asarray(wrapped, dtype=bool).astype(np.int32))
        if np.ndim(nsteps) != 0 or return_distances:
            if np.ndim(nsteps) != 0 and np.shape(nsteps) != (A,):
                raise ValueError("nsteps needs one entry per run (or one int for all)")
            logl_new, ncalls, nclusters, move, pair = self._live_runs_step_steps(runs, kdead, ranks, lstar, wr, nsteps, max_rounds,
                                                                                 seeds, True, nboot, boot_seeds, return_distances,
                                                                                 proposal, step_width)
            return (logl_new, ncalls, nclusters, move, pair) if return_distances else (logl_new, ncalls, nclusters)
        logl_new = np.empty((A, kdead), dtype=np.float64)
        ncalls = np.zeros(A, dtype=np.int64)
        nclusters = np.zeros(A, dtype=np.int32)
        with self._proposal_for(proposal, step_width):
            _abi.check(self._lib.rvll_live_runs_step_clustered(
                self._h, _abi.as_ip(runs), A, kdead, _abi.as_ip(ranks), _abi.as_dp(lstar), _abi.as_ip(wr) if wr is not None else None,
                int(nsteps), int(max_rounds), seeds.ctypes.data_as(C.POINTER(C.c_uint64)), int(nboot),
                boot_seeds.ctypes.data_as(C.POINTER(C.c_uint64)), ncalls.ctypes.data_as(C.POINTER(C.c_int64)), _abi.as_dp(logl_new),
                _abi.as_ip(nclusters)))
        return logl_new, ncalls, nclusters

    def live_runs_clusters(self, a):
        """What the last live_runs_step_clustered found for its listed run a (rvll_live_runs_clusters): (labels [n - kdead] of the
        survivors in rank order, scale [ndim], factors [max(nclusters, 1), ndim, ndim] — the walk's factor of every cluster)."""
        m, k = C.c_int64(0), C.c_int32(0)
        _abi.check(self._lib.rvll_live_runs_clusters(self._h, int(a), C.byref(m), C.byref(k), None, None, None, None))
        labels = np.empty(m.value, dtype=np.int32)
        scale = np.empty(self.ndim)
        factors = np.empty((max(k.value, 1), self.ndim, self.ndim))
        _abi.check(self._lib.rvll_live_runs_clusters(self._h, int(a), None, None, _abi.as_ip(labels), _abi.as_dp(scale),
                                                     _abi.as_dp(factors), None))
        return labels, scale, factors

    def live_runs_cluster_phases(self):
        """Host seconds between the synchronisations of the last clustered step: {"cluster_s", "moments_s", "walk_s"}."""
        ph = np.empty(3)
        _abi.check(self._lib.rvll_live_runs_clusters(self._h, 0, None, None, None, None, None, _abi.as_dp(ph)))
        return {"cluster_s": float(ph[0]), "moments_s": float(ph[1]), "walk_s": float(ph[2])}

    def live_runs_get(self, run, cube=True, theta=True, logl=True, theta_out=None):
        """(cube, theta, logl) of run `run`'s live set as it stands (None for the ones switched off); theta_out: a C-contiguous
        [n, ndim] float64 array (or view) to receive theta in place."""
        self._runs_list([run])
        n = self._runs[1]
        u = np.empty((n, self.ndim)) if cube else None
        th = (theta_out if theta_out is not None else np.empty((n, self.ndim))) if theta else None
        ll = np.empty(n) if logl else None
        if th is not None and (th.shape != (n, self.ndim) or th.dtype != np.float64 or not th.flags.c_contiguous):
            raise ValueError("theta_out must be a C-contiguous float64 array of shape (n, ndim)")
        _abi.check(self._lib.rvll_live_runs_get(self._h, int(run), _abi.as_dp(u) if cube else None,
                                                _abi.as_dp(th) if theta else None, _abi.as_dp(ll) if logl else None))
        return u, th, ll

    def live_runs_dead_count(self, run):
        self._runs_list([run])
        n = C.c_int64(0)
        _abi.check(self._lib.rvll_live_runs_dead(self._h, int(run), C.byref(n), None, None))
        return int(n.value)

    def live_runs_dead(self, run, theta_out=None):
        """(theta, logl) of every point of run `run` that died so far, in the order they died; theta_out: a C-contiguous
        [n_dead, ndim] float64 array (or view) to receive theta in place."""
        n = self.live_runs_dead_count(run)
        th = theta_out if theta_out is not None else np.empty((n, self.ndim))
        if th.shape != (n, self.ndim) or th.dtype != np.float64 or not th.flags.c_contiguous:
            raise ValueError("theta_out must be a C-contiguous float64 array of shape (n_dead, ndim)")
        ll = np.empty(n)
        if n:
            cnt = C.c_int64(n)
            _abi.check(self._lib.rvll_live_runs_dead(self._h, int(run), C.byref(cnt), _abi.as_dp(th), _abi.as_dp(ll)))
        return th, ll

    def live_runs_births(self, run):
        """live_births for run `run` of the resident ensemble (rvll_live_runs_births): (dead in the order live_runs_dead gives,
        live [n])."""
        n = self.live_runs_dead_count(run)
        dead, live = np.empty(n), np.empty(self._runs[1])
        cnt = C.c_int64(n)
        _abi.check(self._lib.rvll_live_runs_births(self._h, int(run), C.byref(cnt), _abi.as_dp(dead), _abi.as_dp(live)))
        return dead, live

    def scalar_server(self, enable=True):
        """Answer scalar log_likelihood(x) calls through a persistent kernel polling pinned host memory (a PCIe
        round trip instead of a launch + synchronisation; same bits).  Any other call on this model stops the
        kernel first; it also leaves by itself after 5 ms without a request and restarts on the next one."""
        _abi.check(self._lib.rvll_scalar_server(self._h, 1 if enable else 0))

    def prior_table_info(self):
        """{parameter: (measured interpolation error, evaluated-by-interpolation flag)} for the Beta/Gamma priors."""
        out = {}
        for d, name in enumerate(self.parnames):
            err, direct = C.c_double(), C.c_int32()
            _abi.check(self._lib.rvll_prior_table_info(self._h, d, C.byref(err), C.byref(direct)))
            if err.value == err.value:
                out[name] = (err.value, bool(direct.value))
        return out

    def dev_prior_loglike(self, n):
        """cube -> theta -> log-L in one launch (the prior transform runs in the log-L kernel's staging step)."""
        _abi.check(self._lib.rvll_dev_prior_loglike(self._h, int(n)))

    def dev_flip_lane(self):
        """Alternate the pipeline lane between independent device-resident batches (include/rvll.h)."""
        return self._lib.rvll_dev_flip_lane(self._h)

    def dev_sync(self):
        _abi.check(self._lib.rvll_dev_sync(self._h))

    def dev_download(self, n, theta=False, logl=True, flags=False):
        n = int(n)
        th = _result_array((n, self.ndim)) if theta else None
        ll = np.empty(n, dtype=np.float64) if logl else None
        fl = np.empty(n, dtype=np.int32) if flags else None
        _abi.check(self._lib.rvll_dev_download(
            self._h, n, _abi.as_dp(th) if theta else None, _abi.as_dp(ll) if logl else None,
            _abi.as_ip(fl) if flags else None))
        return th, ll, fl

    def dev_mark(self, which):
        """Record HIP event 0 (start) or 1 (stop) on the compute stream."""
        _abi.check(self._lib.rvll_dev_mark(self._h, int(which)))

    def dev_mark_elapsed_ms(self):
        ms = C.c_double()
        _abi.check(self._lib.rvll_dev_mark_elapsed(self._h, C.byref(ms)))
        return ms.value

    def dev_time_loglike(self, n, warmup=3, iters=20):
        t = _abi.Timing()
        _abi.check(self._lib.rvll_dev_time_loglike(self._h, int(n), int(warmup), int(iters), C.byref(t)))
        return {f: getattr(t, f) for f, _ in _abi.Timing._fields_}

    def dev_trace_loglike(self, n, warmup=50):
        """Per-workgroup time stamps of one launch of the diagnostic twin of the fp64 kernel (include/rvll.h):
        returns (uint64[blocks, 8], points_per_block)."""
        nb, pb = C.c_int32(), C.c_int32()
        _abi.check(self._lib.rvll_dev_trace_loglike(self._h, int(n), 0, None, 0, C.byref(nb), C.byref(pb)))
        out = np.zeros((nb.value, 8), dtype=np.uint64)
        _abi.check(self._lib.rvll_dev_trace_loglike(self._h, int(n), int(warmup),
                                                    out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size,
                                                    C.byref(nb), C.byref(pb)))
        return out, pb.value

    def set_points_per_block(self, pb):
        _abi.check(self._lib.rvll_set_points_per_block(self._h, int(pb)))

    def set_kernel_form(self, form):
        """Launch form of the log-L kernel: "auto" (by batch size), "tile" or "cu" (include/rvll.h); same bits."""
        _abi.check(self._lib.rvll_set_kernel_form(self._h, {"auto": 0, "tile": 1, "cu": 2}[form]))

    def set_slim_table_range(self, umax):
        """Test hook (include/rvll.h): |logit q| range the table-only prior stage takes before handing over."""
        _abi.check(self._lib.rvll_set_slim_table_range(self._h, float(umax)))

    def set_wander_exact(self, on=True):
        """Redo wandering Kepler solves (e >= 0.97: more than eight Newton steps) with correctly rounded sin / cos (include/rvll.h,
        rvll_set_wander_exact; default on)."""
        _abi.check(self._lib.rvll_set_wander_exact(self._h, 1 if on else 0))

    def set_walk_proposal(self, kind, step_width=1.0):
        """The proposal of every walk on this model from now on (rvll_set_walk_proposal): "chord" (the default:
        hit-and-run along random unit directions, each move shrinking the whole unit-cube chord) or "stepout" (PolyChord's
        stepping out along a cycled random orthonormal basis, brackets step_width whitened units wide; evidence_amd/stepout.py
        is its definition).  The walk methods' proposal= / step_width= keywords override it for one call."""
        kind, step_width = check_proposal(kind, step_width)
        _abi.check(self._lib.rvll_set_walk_proposal(self._h, PROPOSALS.index(kind), step_width))
        self._proposal = (kind, step_width)

    @contextmanager
    def _proposal_for(self, proposal, step_width):
        """A walk method's proposal= / step_width= (None: the model's own, set_walk_proposal): set on the handle for the call
        and put back after it."""
        if proposal is None and step_width is None:
            yield
            return
        own = getattr(self, "_proposal", ("chord", 1.0))
        kind, width = check_proposal(own[0] if proposal is None else proposal, own[1] if step_width is None else step_width)
        _abi.check(self._lib.rvll_set_walk_proposal(self._h, PROPOSALS.index(kind), width))
        try:
            yield
        finally:
            _abi.check(self._lib.rvll_set_walk_proposal(self._h, PROPOSALS.index(own[0]), own[1]))

    def set_walk_speculation(self, max_ahead):
        """Candidates a walker of slice_walk may evaluate ahead per iteration in otherwise free tile slots (include/rvll.h;
        default 4, 1 = none).  Results do not depend on it."""
        _abi.check(self._lib.rvll_set_walk_speculation(self._h, int(max_ahead)))

    def slice_walk_evaluated(self):
        """Tile slots the last slice_walk evaluated (>= the calls it reported: unused speculative candidates included)."""
        n = C.c_int64(0)
        _abi.check(self._lib.rvll_slice_walk_evaluated(self._h, C.byref(n)))
        return int(n.value)

    def slice_walk_rounds(self):
        """Rounds the last slice_walk / live_step took in the rounds form (include/rvll.h); 0: a single-kernel form walked."""
        n = C.c_int32(0)
        _abi.check(self._lib.rvll_slice_walk_rounds(self._h, C.byref(n)))
        return int(n.value)

    def slice_walk_phases(self):
        """Diagnostic library build only (include/rvll.h): ticks per phase of the last slice_walk, summed over workgroups."""
        out = (C.c_uint64 * 6)()
        _abi.check(self._lib.rvll_slice_walk_phases(self._h, out))
        return [int(v) for v in out]

    def debug_eval(self, op, x, y=None):
        """Evaluate one device math routine elementwise (include/rvll.h, diagnostics)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        yy = None if y is None else np.ascontiguousarray(np.broadcast_to(y, x.shape), dtype=np.float64)
        out = np.empty_like(x)
        _abi.check(self._lib.rvll_debug_eval(self._h, int(op), _abi.as_dp(x), _abi.as_dp(yy) if yy is not None else None,
                                             x.size, _abi.as_dp(out)))
        return out

    # ---- multi-GPU ----------------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = (C.c_ubyte * _abi.COMM_ID_BYTES)()
        _abi.check(_abi.load().rvll_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, comm_id: bytes, nranks: int, rank: int):
        if len(comm_id) != _abi.COMM_ID_BYTES:
            raise ValueError("comm id must be 128 bytes")
        buf = (C.c_ubyte * _abi.COMM_ID_BYTES).from_buffer_copy(comm_id)
        _abi.check(self._lib.rvll_comm_init(self._h, buf, int(nranks), int(rank)))

    def comm_add_lanes(self, want=3):
        """Collective: try to add pipeline lanes (ncclCommSplit); returns how many this rank holds.  The ranks must
        agree on the minimum and call comm_set_lanes with it (include/rvll.h)."""
        have = C.c_int32(1)
        _abi.check(self._lib.rvll_comm_add_lanes(self._h, int(want), C.byref(have)))
        return have.value

    def comm_set_lanes(self, n):
        _abi.check(self._lib.rvll_comm_set_lanes(self._h, int(n)))

    def allgather_host(self, mine, world):
        """RCCL all-gather of a small float64 host array: [n] per rank -> [world, n] on every rank."""
        mine = np.ascontiguousarray(mine, dtype=np.float64).ravel()
        out = np.empty((int(world), mine.size), dtype=np.float64)
        _abi.check(self._lib.rvll_allgather_host(self._h, _abi.as_dp(mine), mine.size, _abi.as_dp(out)))
        return out

    @staticmethod
    def runtime_info():
        """Which HIP runtime / RCCL / librvll this process runs on (include/rvll.h rvll_runtime_info)."""
        import json
        buf = C.create_string_buffer(2048)
        _abi.check(_abi.load().rvll_runtime_info(buf, len(buf)))
        info = json.loads(buf.value.decode())
        info["hw_queues"] = _abi.HW_QUEUES_NOTE           # set by evidence_amd at load time? in effect?
        return info

    def allgather_logl(self, n_local):
        _abi.check(self._lib.rvll_allgather_logl(self._h, int(n_local)))

    def download_gathered(self, n_total):
        out = np.empty(int(n_total), dtype=np.float64)
        _abi.check(self._lib.rvll_download_gathered(self._h, int(n_total), _abi.as_dp(out)))
        return out

    def allgather_theta(self, n_local):
        """All-gather the resident theta rows (produced on the device by the prior transform) of every rank."""
        _abi.check(self._lib.rvll_allgather_theta(self._h, int(n_local)))

    def download_gathered_theta(self, n_total):
        out = np.empty((int(n_total), self.ndim), dtype=np.float64)
        _abi.check(self._lib.rvll_download_gathered_theta(self._h, int(n_total), _abi.as_dp(out)))
        return out

    def comm_destroy(self):
        _abi.check(self._lib.rvll_comm_destroy(self._h))
