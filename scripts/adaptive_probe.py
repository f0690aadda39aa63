#!/usr/bin/env python3
"""Does the step-count adaptation (adaptive_nsteps="move-distance") change what the insertion-index test finds on the
51 Peg resident ensembles?  R independent clustered resident runs of examples/51peg/config_51peg.py (k = 1 and 2
planets, 400 live points, kbatch 100, dlogz 0.5, nsteps = 3 ndim), adaptation off and on (min_nsteps = nsteps, max_nsteps 1000).
Per setting:
    lnZ sd / iqr     the spread of ln Z over the runs
    fail             runs that fail insertion.test(device=0) at alpha = 0.01; deaths: the median deaths before the first failing window
    shrink           the mean simulated-shrinkage ln Z error (shrinkage.logz_error, device=0)
    calls, wall      likelihood calls over all runs, and the ensemble's wall time
    nsteps           quantiles (10, 50, 90 %, max) of the step counts the runs' iterations walked with
--kernel-only R k: one adaptive clustered ensemble and nothing else (the run to put under rocprofv3 --kernel-trace --stats for the
distance pass's kernel time).  Run on the GPU box:
    python3 scripts/adaptive_probe.py [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, insertion, run_nested_ensemble, shrinkage  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

ALPHA = 0.01
CFG = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"


def _model(k):
    rundict, datadict, priordict, fixed = read_config(CFG, nplanets=k)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def main(R):
    print(f"51 Peg resident ensembles, clustered, R = {R}, 400 live points, kbatch 100; insertion test alpha = {ALPHA}", flush=True)
    print(f"{'k':>2} {'adaptive':>8} {'lnZ sd':>7} {'lnZ iqr':>7} {'fail':>5} {'deaths':>7} {'shrink':>7} {'calls':>10} {'wall':>7} "
          f"{'nsteps p10/p50/p90/max':>24}", flush=True)
    for k in (1, 2):
        with _model(k) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=200_000_000, clustering=True)
            run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)                       # kernels loaded
            for adaptive in (None, "move-distance"):
                t0 = time.perf_counter()
                got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, adaptive_nsteps=adaptive, **kw)
                wall = time.perf_counter() - t0
                logz = np.array([g.logz for g in got])
                recs = insertion.test(got, device=0, alpha=ALPHA)["runs"]
                fail = [r for r in recs if r["failed"]]
                deaths = [r["first_window_deaths"] for r in fail if r["first_window_deaths"] is not None]
                err = shrinkage.logz_error(got, device=0)
                steps = (np.concatenate([g.nsteps_trace for g in got]) if adaptive
                         else np.full(1, 3 * m.ndim))
                q = np.percentile(steps, [10, 50, 90])
                print(f"{k:>2} {str(adaptive is not None):>8} {np.std(logz):>7.2f} {np.subtract(*np.percentile(logz, [75, 25])):>7.2f} "
                      f"{len(fail):>5} {np.median(deaths) if deaths else float('nan'):>7.0f} {np.mean(err):>7.2f} "
                      f"{sum(g.ncall for g in got):>10} {wall:>6.1f}s {q[0]:>5.0f}/{q[1]:.0f}/{q[2]:.0f}/{steps.max():.0f}", flush=True)


def kernel_only(R, k):
    with _model(k) as m:
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=200_000_000, clustering=True)
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, adaptive_nsteps="move-distance", **kw)
        print(f"k = {k}, R = {R}: {sum(len(g.nsteps_trace) for g in got)} run-iterations measured", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--kernel-only"]:
        kernel_only(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
