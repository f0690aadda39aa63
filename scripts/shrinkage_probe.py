#!/usr/bin/env python3
"""Sampler scatter against statistical scatter: R independent resident runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5), with and without clustering,
for R = 32 and 128 (or the R given).  Per setting:
    spread          the standard deviation of ln Z across the R runs
    replicates      the mean over runs of the standard deviation of ln Z over S = 1000 simulated-shrinkage replicates
    sqrt(H/nlive)   the mean of the drivers' logzerr
    GPU             rvll_shrinkage_replicates for all R runs, S = 1000: kernel (HIP events) and whole call
    numpy           the definition (shrinkage.replicates, device=None), timed on the first 4 runs and scaled by R / 4
--gpu-only skips the numpy timing (the run to put under rocprofv3 --kernel-trace --stats).  Run on the GPU box:
    python3 scripts/shrinkage_probe.py [--gpu-only] [R ...]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, run_nested_ensemble, shrinkage  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_RUNS = 4


def main(rs, gpu_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    print(f"simulated shrinkage, S = {S} replicates per run; ln Z in nats", flush=True)
    print(f"{'k':>2} {'R':>4} {'clustering':>10} {'deaths/run':>10} {'median lnZ':>11} {'spread':>8} {'replicates':>10} "
          f"{'sqrt(H/n)':>9} {'GPU kernel':>11} {'GPU call':>9} {'numpy':>9}", flush=True)
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            warm = run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)
            shrinkage.replicates(warm, nsamples=8, device=0)                       # kernels loaded
            for R in rs:
                for clustering in (False, True):
                    got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=clustering, **kw)
                    logz = np.array([g.logz for g in got])
                    timing = {}
                    reps, _ = shrinkage.replicates(got, nsamples=S, seed=1, device=0, timing=timing)
                    numpy_s = float("nan")
                    if not gpu_only:
                        t0 = time.perf_counter()
                        ref, _ = shrinkage.replicates(got[:NUMPY_RUNS], nsamples=S, seed=shrinkage.keep_words(1, R)[:NUMPY_RUNS])
                        numpy_s = (time.perf_counter() - t0) * R / NUMPY_RUNS
                        assert np.max(np.abs(ref - reps[:NUMPY_RUNS])) <= 1e-9
                    deaths = np.mean([g.niter for g in got])
                    print(f"{k:>2} {R:>4} {str(clustering):>10} {deaths:>10.0f} {np.median(logz):>11.2f} {np.std(logz):>8.3f} "
                          f"{np.mean(np.std(reps, axis=1)):>10.3f} {np.mean([g.logzerr for g in got]):>9.3f} "
                          f"{timing['kernel_ms']:>8.2f} ms {timing['total_ms']:>6.1f} ms {numpy_s:>7.1f} s", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main([int(a) for a in args] or [32, 128], "--gpu-only" in sys.argv[1:])
