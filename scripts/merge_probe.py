#!/usr/bin/env python3
"""Merged runs against single runs: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5) merged by their birth contours.
Per k:
    merged lnZ      merge.merge (expected shrinkage, device 0)
    shrink sd       the standard deviation of ln Z over S = 1000 simulated-shrinkage replicates of the merged run
    boot sd         the same with the runs resampled with replacement in every replicate (Higson et al. 2018 §4)
    single runs     the median of the R drivers' ln Z, their standard deviation, and that over sqrt(R)
    GPU             rvll_merge_replicates, S = 1000 with the bootstrap: kernels (HIP events) and the whole call
    numpy           the definition (merge.replicates, device=None) timed on NUMPY_REPS replicates and scaled to S
--gpu-only skips the numpy timing (the run to put under rocprofv3 --kernel-trace --stats).  Run on the GPU box:
    python3 scripts/merge_probe.py [--gpu-only] [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, merge, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_REPS = 2


def main(R, gpu_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    print(f"merged runs, S = {S} replicates; ln Z in nats", flush=True)
    print(f"{'k':>2} {'R':>4} {'rows':>8} {'merged lnZ':>11} {'shrink sd':>9} {'boot sd':>8} {'median lnZ':>11} {'spread':>7} "
          f"{'spread/sqR':>10} {'off-c':>5} {'GPU kernel':>11} {'GPU call':>9} {'numpy':>9}", flush=True)
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            warm = run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)
            merge.replicates(warm, nsamples=8, device=0)                         # kernels loaded
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw)
        logz = np.array([g.logz for g in got])
        _, logl, birth, run_start = merge._stack(got)
        one = merge.merge_arrays(logl, birth, run_start, device=0)
        shrink, _ = merge.replicates(got, nsamples=S, seed=1, bootstrap=False, device=0)
        timing = {}
        boot, _ = merge.replicates(got, nsamples=S, seed=1, bootstrap=True, device=0, timing=timing)
        numpy_s = float("nan")
        if not gpu_only:
            t0 = time.perf_counter()
            ref, _ = merge.replicates(got, nsamples=NUMPY_REPS, seed=1, bootstrap=True)
            numpy_s = (time.perf_counter() - t0) * S / NUMPY_REPS
            err = np.max(np.abs(ref - boot[:NUMPY_REPS]) / np.abs(ref))
            print(f"   (device against the definition on the first {NUMPY_REPS} bootstrap replicates: max rel err {err:.1e})",
                  flush=True)
        print(f"{k:>2} {R:>4} {logl.size:>8} {one['logz']:>11.3f} {np.std(shrink):>9.4f} {np.std(boot):>8.4f} "
              f"{np.median(logz):>11.2f} {np.std(logz):>7.3f} {np.std(logz) / np.sqrt(R):>10.4f} {one['off_contour']:>5} "
              f"{timing['kernel_ms']:>8.2f} ms {timing['total_ms']:>6.1f} ms {numpy_s:>7.1f} s", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main(int(args[0]) if args else 128, "--gpu-only" in sys.argv[1:])
