#!/usr/bin/env python3
"""Which runs of a resident ensemble does the insertion-index test flag?  R independent resident runs of the 51 Peg
example (examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5), with and without
clustering, for R = 32 and 128 (or the R given).  Per setting:
    fail            runs that fail the test at alpha = 0.01 (whole run, or a window of 400 insertions below alpha / windows)
    |dlnZ| fail/ok  the mean distance of ln Z from the median over the R runs, for the failing and the passing runs
    pooled p        the KS p-value of all runs' ranks together
    off-schedule    inserted rows whose live set did not hold nlive points (born on a tied contour), summed over the runs
    off-contour     rows whose log-L the exact redo lowered to their birth contour or below, summed over the runs
    GPU             rvll_insertion_indexes for all R runs: kernel (HIP events) and whole call
    numpy           the definition (insertion.indexes_arrays, device=None) on the first 4 runs, scaled by R / 4
and per run (every run for R = 32, the failing runs for larger R): ln Z, n, D, p and the first failing window (its birth contour
and the deaths before it).  --gpu-only skips the numpy timing (the run to put under rocprofv3 --kernel-trace --stats).  Run on
the GPU box:
    python3 scripts/insertion_probe.py [--gpu-only] [R ...]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, insertion, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

NUMPY_RUNS = 4
ALPHA = 0.01


def _fmt_window(rec):
    if rec["first_window"] is None:
        return "-"
    return f"#{rec['first_window']} at logL {rec['first_window_birth']:.2f} after {rec['first_window_deaths']} deaths"


def main(rs, gpu_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    print(f"insertion-index test, alpha = {ALPHA}, windows of nlive = 400 insertions; ln Z in nats", flush=True)
    print(f"{'k':>2} {'R':>4} {'clustering':>10} {'rows/run':>8} {'fail':>5} {'|dlnZ| fail':>11} {'|dlnZ| ok':>9} "
          f"{'pooled p':>9} {'off-schedule':>12} {'off-contour':>11} {'GPU kernel':>11} {'GPU call':>9} {'numpy':>8}", flush=True)
    per_run = []
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            warm = run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)
            insertion.indexes(warm, device=0)                                        # kernels loaded
            for R in rs:
                for clustering in (False, True):
                    got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=clustering, **kw)
                    logz = np.array([g.logz for g in got])
                    timing = {}
                    out = insertion.test(got, device=0, alpha=ALPHA, timing=timing)
                    numpy_s = float("nan")
                    if not gpu_only:
                        sub = got[:NUMPY_RUNS]
                        logl = np.concatenate([g.logl for g in sub])
                        birth = np.concatenate([g.logl_birth for g in sub])
                        rs_ = np.concatenate([[0], np.cumsum([len(g.logl) for g in sub])])
                        t0 = time.perf_counter()
                        ref = insertion.indexes_arrays(logl, birth, rs_)
                        numpy_s = (time.perf_counter() - t0) * R / NUMPY_RUNS
                        dev = insertion.indexes_arrays(logl, birth, rs_, device=0)
                        assert np.array_equal(ref[0], dev[0]) and np.array_equal(ref[1], dev[1])
                    recs = out["runs"]
                    fail = np.array([r["failed"] for r in recs])
                    dist = np.abs(logz - np.median(logz))
                    df = np.mean(dist[fail]) if fail.any() else float("nan")
                    dok = np.mean(dist[~fail]) if (~fail).any() else float("nan")
                    offc = sum(r["off_contour"] for r in recs)
                    offs = sum(r["off_schedule"] for r in recs)
                    print(f"{k:>2} {R:>4} {str(clustering):>10} {np.mean([len(g.logl) for g in got]):>8.0f} {int(fail.sum()):>5} "
                          f"{df:>11.2f} {dok:>9.2f} {out['pooled']['pvalue']:>9.2e} {offs:>12} {offc:>11} {timing['kernel_ms']:>8.2f} ms "
                          f"{timing['total_ms']:>6.1f} ms {numpy_s:>6.1f} s", flush=True)
                    for s, (g, rec) in enumerate(zip(got, recs), start=1):
                        if R <= 32 or rec["failed"]:
                            per_run.append(f"{k:>2} {R:>4} {str(clustering):>10} {s:>4} {g.logz:>9.2f} {rec['n']:>6} {rec['D']:>7.4f} "
                                           f"{rec['pvalue']:>9.2e} {'FAIL' if rec['failed'] else 'ok':>4}  {_fmt_window(rec)}")
    print("\nper run (seed = run number):", flush=True)
    print(f"{'k':>2} {'R':>4} {'clustering':>10} {'seed':>4} {'lnZ':>9} {'n':>6} {'D':>7} {'p':>9} {'test':>4}  first failing window",
          flush=True)
    for line in per_run:
        print(line, flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main([int(a) for a in args] or [32, 128], "--gpu-only" in sys.argv[1:])
