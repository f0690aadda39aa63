#!/usr/bin/env python3
"""Posterior summaries of merged runs with both error bars: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5), every parameter summarised over
S = 1000 replicates with the run bootstrap (k = 2: planets ordered by period first).  Per k, medians of REPEATS calls after a
warm-up call:
    weights alone   merge.replicates(device=0): rvll_merge_replicates on the same rows, no weights returned — what producing
                    the replicated weights costs (the entry is unchanged by the posterior work)
    summaries       posterior.summarize_arrays(device=0): rvll_posterior_replicates — HIP-event time in all and of its three
                    parts (setup: merge setup, permutation, one radix sort a column; weights: the replicate kernels; reduce:
                    exp and the summary kernel), the whole C call, and the wall time of the Python call
    numpy           the definition (device=None) timed on NUMPY_REPS replicates and scaled to S (labelled as scaled)
then the table: point estimates from the expected weights, and per entry the bootstrap error next to the shrinkage-only error.
Run on the GPU box:  python3 scripts/posterior_probe.py [--gpu-only] [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, merge, posterior, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_REPS = 2
REPEATS = 5


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def main(R, gpu_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            names = list(m.parnames)
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            warm = run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)
            merge.replicates(warm, nsamples=8, device=0)                         # kernels loaded
            posterior.summarize(warm, nsamples=8, device=0)
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw)
        _, cols, logl, birth, run_start = posterior._values(got, None, None, k > 1, names)
        n, ncols = cols.shape
        posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=S, seed=1, device=0)      # warm-up at the timed shape
        merge.replicates_arrays(logl, birth, run_start, S, seed=1, device=0)
        mt, pt, wall = [], [], []
        for _ in range(REPEATS):                                                 # the two entries alternate
            t = {}
            merge.replicates_arrays(logl, birth, run_start, S, seed=1, device=0, timing=t)
            mt.append(t)
            t = {}
            t0 = time.perf_counter()
            dev = posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=S, seed=1, device=0, timing=t)
            wall.append(1e3 * (time.perf_counter() - t0))
            pt.append(t)
        print(f"k = {k}: R = {R} runs, {n} merged rows, {ncols} columns, S = {S} replicates, 3 quantile levels; "
              f"medians of {REPEATS} calls (min .. max of the kernel time)", flush=True)
        print(f"  weights alone (rvll_merge_replicates):   kernels {med(mt, 'kernel_ms'):9.2f} ms "
              f"({min(r['kernel_ms'] for r in mt):.2f} .. {max(r['kernel_ms'] for r in mt):.2f})   call {med(mt, 'total_ms'):9.1f} ms")
        print(f"  summaries (rvll_posterior_replicates):   kernels {med(pt, 'kernel_ms'):9.2f} ms "
              f"({min(r['kernel_ms'] for r in pt):.2f} .. {max(r['kernel_ms'] for r in pt):.2f})   call {med(pt, 'total_ms'):9.1f} ms"
              f"   Python call {float(np.median(wall)):9.1f} ms")
        print(f"      setup {med(pt, 'setup_ms'):8.2f} ms   weights {med(pt, 'weights_ms'):8.2f} ms   reduce "
              f"{med(pt, 'reduce_ms'):8.2f} ms   in {pt[0]['blocks']} blocks of replicates, {pt[0]['launches']} launches")
        rate = n * S * ncols / (med(pt, "reduce_ms") * 1e-3)
        print(f"      reduce: {rate / 1e9:.1f}e9 (row, replicate, column) triples a second; each is read in three passes, one a "
              f"gather", flush=True)
        for gib in (0.5, 2.0, 8.0):                                              # the block of weights next to the tables
            rows = []
            for _ in range(3):
                t = {}
                posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=S, seed=1, device=0, timing=t,
                                           block_bytes=posterior.table_bytes(n, ncols) + int(gib * 2 ** 30))
                rows.append(t)
            print(f"      weights block {gib:4.1f} GiB: {rows[0]['blocks']:3d} blocks   weights {med(rows, 'weights_ms'):8.2f} ms   "
                  f"reduce {med(rows, 'reduce_ms'):8.2f} ms   kernels {med(rows, 'kernel_ms'):8.2f} ms", flush=True)
        if not gpu_only:
            t0 = time.perf_counter()
            ref = posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=NUMPY_REPS, seed=1)
            numpy_s = (time.perf_counter() - t0) * S / NUMPY_REPS
            same = int((ref["quantiles"] == dev["quantiles"][:NUMPY_REPS]).sum())
            err = np.max(np.abs(ref["mean"] - dev["mean"][:NUMPY_REPS]) / np.abs(ref["mean"]))
            print(f"  numpy definition: {numpy_s:.0f} s scaled from {NUMPY_REPS} replicates (x {S // NUMPY_REPS}); device "
                  f"against it there: {same} of {ref['quantiles'].size} quantiles equal, max rel err of a mean {err:.1e}")
        boot = posterior.table(got, names, order=k > 1, nsamples=S, seed=1, device=0)
        shrink = posterior.table(got, names, order=k > 1, nsamples=S, seed=1, device=0, bootstrap=False)
        print(posterior.format_table(boot, other=shrink, labels=("boot", "shrink")), flush=True)
        print(flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main(int(args[0]) if args else 128, "--gpu-only" in sys.argv[1:])
