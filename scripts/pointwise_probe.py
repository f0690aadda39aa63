#!/usr/bin/env python3
"""Pointwise predictive checks of merged runs: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, dlogz 0.5), lpd, WAIC and LOO per epoch and per night over
S = 1000 replicates with the run bootstrap.  Per k and per grouping, medians of REPEATS calls after a warm-up call:
    pointwise       pointwise.pointwise_arrays(device=0): rvll_pointwise_replicates — HIP-event time of its three parts (setup:
                    merge setup and the operand B; weights: the replicate kernels; reduce: exp of the block, the fp64 MFMA
                    product and the kernel that adds the slabs), the whole C call and the wall time of the Python call, which
                    holds the host's shifts
    share of peak   2 S N C operations (C = 4 U + 1 columns) over reduce_ms against 78.6 TF, the data-sheet fp64 matrix peak;
                    reduce_ms holds exp and the slab sums as well, so the product alone is a little above the figure
    per column      rvll_posterior_replicates on the first 64 units as values with one quantile level: its reduce_ms, scaled by
                    C / 64 (labelled as scaled) — the per-(replicate, column) reducer that the project had for the same columns
    numpy           the definition (device=None) on NUMPY_REPS replicates of NUMPY_UNITS units, scaled to S and U (labelled)
then the totals with their errors, the units that the model predicts worst, and compare(k = 1, k = 2).
Run on the GPU box:  python3 scripts/pointwise_probe.py [--gpu-only] [--k 1|2] [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, pointwise, posterior, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_REPS = 1
NUMPY_UNITS = 16
REPEATS = 3
PEAK_TF = 78.6


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def probe(name, table, logl, birth, run_start, gpu_only):
    n, units = table.shape
    cols = 4 * units + 1
    kw = dict(nsamples=S, seed=1, device=0)
    pointwise.pointwise_arrays(table, logl, birth, run_start, **kw)                # warm-up at the timed shape
    rows, wall = [], []
    for _ in range(REPEATS):
        t = {}
        t0 = time.perf_counter()
        dev = pointwise.pointwise_arrays(table, logl, birth, run_start, timing=t, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        rows.append(t)
    t0 = time.perf_counter()
    pointwise.shifts_of(table, logl, birth, run_start)
    shifts_ms = 1e3 * (time.perf_counter() - t0)
    red = med(rows, "reduce_ms")
    print(f"  {name}: U = {units} units, C = {cols} columns, {rows[0]['slabs']} slabs of {pointwise.slab_rows()} rows, "
          f"{rows[0]['blocks']} blocks of replicates, {rows[0]['unit_blocks']} block of units, {rows[0]['launches']} launches")
    print(f"    pointwise (rvll_pointwise_replicates):  setup {med(rows, 'setup_ms'):9.2f} ms   weights {med(rows, 'weights_ms'):9.2f} ms   "
          f"reduce {red:9.2f} ms ({min(r['reduce_ms'] for r in rows):.2f} .. {max(r['reduce_ms'] for r in rows):.2f})   "
          f"call {med(rows, 'total_ms'):9.1f} ms   Python call {float(np.median(wall)):9.1f} ms, of which the host's shifts "
          f"{shifts_ms:.0f} ms")
    flop = 2.0 * S * n * cols
    print(f"    reduce: {flop:.3e} operations (2 S N C) in {red:.2f} ms = {flop / (red * 1e-3) / 1e12:.2f} TF = "
          f"{100.0 * flop / (red * 1e-3) / 1e12 / PEAK_TF:.1f} % of {PEAK_TF} TF", flush=True)
    ncol = min(units, posterior.MAX_COLUMNS)
    values = np.ascontiguousarray(table[:, :ncol])
    posterior.summarize_arrays(values, logl, birth, run_start, quantiles=[0.5], **kw)
    prow = []
    for _ in range(REPEATS):
        t = {}
        posterior.summarize_arrays(values, logl, birth, run_start, quantiles=[0.5], timing=t, **kw)
        prow.append(t)
    pred = med(prow, "reduce_ms")
    print(f"    per column (rvll_posterior_replicates, {ncol} columns, one quantile level): reduce {pred:.2f} ms, setup "
          f"{med(prow, 'setup_ms'):.2f} ms; scaled to {cols} columns (x {cols / ncol:.2f}): reduce {pred * cols / ncol:.0f} ms = "
          f"{pred * cols / ncol / red:.1f} times the product's", flush=True)
    if not gpu_only:
        nu = min(units, NUMPY_UNITS)
        sub = np.ascontiguousarray(table[:, :nu])
        t0 = time.perf_counter()
        ref = pointwise.pointwise_arrays(sub, logl, birth, run_start, nsamples=NUMPY_REPS, seed=1)
        numpy_s = (time.perf_counter() - t0) * (S / NUMPY_REPS) * (units / nu)
        err = max(float(np.max(np.abs(ref[k] - dev[k][:NUMPY_REPS, :nu]))) for k in ("lpd", "loo"))
        print(f"    numpy definition: {numpy_s:.0f} s scaled from {NUMPY_REPS} replicate of {nu} units (x {S // NUMPY_REPS} x "
              f"{units / nu:.1f}); device against it there: max |lpd, loo err| {err:.1e}", flush=True)
    return dev


def report(name, res, time_of_unit):
    print(f"  {name}: lpd {res['lpd_total']:.3f} +/- {res['lpd_total_err']:.3f}   waic {res['waic_total']:.3f} +/- "
          f"{res['waic_total_err']:.3f}   loo {res['loo_total']:.3f} +/- {res['loo_total_err']:.3f}   p_waic "
          f"{res['p_waic_total']:.2f}   smallest loo_ess {res['loo_ess'].min():.0f}   most truncated rows "
          f"{int(res['truncated_rows'].max())} of {res['table'].shape[0]}")
    worst = np.argsort(res["loo"])[:5]
    print("    the five units predicted worst (unit, first epoch, loo +/- err, lpd - loo): " + "; ".join(
        f"{u} t={time_of_unit[u]:.2f} {res['loo'][u]:.3f} +/- {res['loo_err'][u]:.3f} {res['lpd'][u] - res['loo'][u]:.3f}"
        for u in worst), flush=True)


def main(R, gpu_only, ks):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    results = {}
    for k in ks:
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            warm = run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)
            pointwise.loo(warm, m, nsamples=8, device=0)                           # kernels loaded
            t0 = time.perf_counter()
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw)
            print(f"k = {k}: the {R} runs took {time.perf_counter() - t0:.0f} s", flush=True)
            samples, logl, birth, run_start = pointwise._samples(got)
            t0 = time.perf_counter()
            per_epoch = pointwise.unit_loglik(m, samples)
            table_s = time.perf_counter() - t0
            nights = pointwise.by_night(m.table.time)
            per_night = pointwise.unit_loglik(m, samples, nights)
            epoch_time = np.asarray(m.table.time, dtype=np.float64)
        night_time = np.array([epoch_time[nights == u].min() for u in range(nights.max() + 1)])
        print(f"k = {k}: R = {R} runs, {logl.size} merged rows, {per_epoch.shape[1]} epochs in {per_night.shape[1]} nights, S = {S} "
              f"replicates with the run bootstrap; medians of {REPEATS} calls (min .. max).  The table of unit log-likelihoods "
              f"(residuals on the device, the rest in numpy): {table_s:.1f} s", flush=True)
        probe("per epoch", per_epoch, logl, birth, run_start, gpu_only)
        probe("per night", per_night, logl, birth, run_start, gpu_only)
        results[k] = (pointwise.loo(got, None, nsamples=S, seed=1, device=0, table=per_epoch),
                      pointwise.loo(got, None, nsamples=S, seed=1, device=0, table=per_night))
        report("per epoch", results[k][0], epoch_time)
        report("per night", results[k][1], night_time)
        print(flush=True)
    if 1 in results and 2 in results:
        for name, i in (("per epoch", 0), ("per night", 1)):
            c = pointwise.compare(results[2][i], results[1][i])
            print(f"compare(k = 2, k = 1) {name}: elpd_loo difference {c['elpd_diff']:.3f}, error from the replicates "
                  f"{c['err_replicates']:.3f}, between-unit standard error {c['err_units']:.3f}")


if __name__ == "__main__":
    argv = sys.argv[1:]
    ks = (1, 2)
    if "--k" in argv:
        i = argv.index("--k")
        ks = (int(argv[i + 1]),)
        del argv[i:i + 2]
    args = [a for a in argv if a != "--gpu-only"]
    main(int(args[0]) if args else 128, "--gpu-only" in argv, ks)
