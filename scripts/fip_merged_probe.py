#!/usr/bin/env python3
"""The FIP periodogram of merged runs with run-to-run error bars: R = 128 resident clustered runs of the 51 Peg
example (examples/51peg/config_51peg.py, k = 0, 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5), the reference's grid
of 50 000 frequencies, S = 1000 replicates with the run bootstrap.  Per planet model, medians of REPEATS calls after a warm-up:
    periodogram     fip.merged_tip_arrays(device=0): rvll_fip_replicates — HIP-event time in all and of its three parts (setup:
                    merge setup, spans, two radix sorts, tables; weights: the replicate kernels; reduce: exp and P, the coverage
                    kernel, the TIP kernel), the whole C call and the wall time of the Python call
    yardstick       posterior.summarize_arrays(device=0) on the same rows with 2 np columns (the periods twice): the same
                    number of gathers a replicate
    numpy           the definition (device=None) timed on NUMPY_REPS replicates and scaled to S (labelled as scaled)
then what the numbers say: p(k | y) and log10 FIP at the 4.23 d peak with the bootstrap error, the shrinkage-only error
(bootstrap=False) and the spread of the per-run curves (fip.fip_periodogram / fip_summary), and the host time of merged_fip.
With --kernels-only the script makes one call a model and nothing else: run it under `rocprofv3 --kernel-trace --stats` for the
time of every kernel.
Run on the GPU box:  python3 scripts/fip_merged_probe.py [--gpu-only | --kernels-only] [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, fip, merge, posterior, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_REPS = 2
REPEATS = 3


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def main(R, gpu_only, kernels_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    models, cols, datadict = [], [], None
    for k in (0, 1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            models.append(run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw))
            cols.append([m.parnames.index(f"planet{j}_period") for j in range(1, k + 1)])
    nu, nua, nub = fip.frequency_grid(1.5, 1000.0, fip.observation_span(datadict))
    for k in (1, 2):
        _, logl, birth, run_start = merge._stack(models[k])
        per = np.ascontiguousarray(np.concatenate([np.asarray(r.samples)[:, cols[k]] for r in models[k]]))
        n = logl.size
        fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=S, seed=1, device=0)          # warm-up
        if kernels_only:
            continue
        two = np.concatenate([per, per], axis=1)
        posterior.summarize_arrays(two, logl, birth, run_start, nsamples=S, seed=1, device=0)
        ft, pt, wall = [], [], []
        for _ in range(REPEATS):
            t = {}
            t0 = time.perf_counter()
            dev = fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=S, seed=1, device=0, timing=t)
            wall.append(1e3 * (time.perf_counter() - t0))
            ft.append(t)
            t = {}
            posterior.summarize_arrays(two, logl, birth, run_start, nsamples=S, seed=1, device=0, timing=t)
            pt.append(t)
        print(f"k = {k}: R = {R} runs, {n} merged rows, {nu.size} bins, S = {S} replicates; medians of {REPEATS} calls "
              f"(min .. max of the kernel time)", flush=True)
        print(f"  periodogram (rvll_fip_replicates):      kernels {med(ft, 'kernel_ms'):9.2f} ms "
              f"({min(r['kernel_ms'] for r in ft):.2f} .. {max(r['kernel_ms'] for r in ft):.2f})   call {med(ft, 'total_ms'):9.1f} ms"
              f"   Python call {float(np.median(wall)):9.1f} ms")
        print(f"      setup {med(ft, 'setup_ms'):8.2f} ms   weights {med(ft, 'weights_ms'):8.2f} ms   reduce "
              f"{med(ft, 'reduce_ms'):8.2f} ms   in {ft[0]['blocks']} blocks of replicates, {ft[0]['launches']} launches, "
              f"{ft[0]['events']} events, {ft[0]['key_bits']} key bits")
        print(f"  yardstick (rvll_posterior_replicates, {2 * k} columns): kernels {med(pt, 'kernel_ms'):9.2f} ms   setup "
              f"{med(pt, 'setup_ms'):8.2f} ms   weights {med(pt, 'weights_ms'):8.2f} ms   reduce {med(pt, 'reduce_ms'):8.2f} ms",
              flush=True)
        if not gpu_only:
            t0 = time.perf_counter()
            ref = fip.merged_tip_arrays(per, logl, birth, run_start, nua, nub, nsamples=NUMPY_REPS, seed=1)
            numpy_s = (time.perf_counter() - t0) * S / NUMPY_REPS
            err = float(np.max(np.abs(ref["tip"] - dev["tip"][:NUMPY_REPS])))
            print(f"  numpy definition: {numpy_s:.0f} s scaled from {NUMPY_REPS} replicates (x {S // NUMPY_REPS}); device "
                  f"against it there: max |tip difference| {err:.1e}", flush=True)
    if kernels_only:
        return
    out = {}
    for label, boot in (("bootstrap", True), ("shrinkage", False)):
        t, t0 = {}, time.perf_counter()
        out[label] = fip.merged_fip(models, cols, nua, nub, nsamples=S, seed=1, bootstrap=boot, device=0, nu=nu, timing=t)
        wall = time.perf_counter() - t0
        print(f"merged_fip, {label}: {wall:.2f} s on the host, of which {1e-3 * t['total_ms']:.2f} s in the C calls "
              f"({1e-3 * t['kernel_ms']:.2f} s kernels)")
    boot, shrink = out["bootstrap"], out["shrinkage"]
    best = int(np.argmin(boot["log10fip"]))
    logzs = np.array([[r.logz for r in models[k]] for k in range(3)]).T
    pky = fip.model_probabilities(logzs)
    posteriors = [[None] + [(np.asarray(models[k][r].samples)[:, cols[k]], np.exp(models[k][r].logwt)) for k in (1, 2)]
                  for r in range(R)]
    s = fip.fip_summary(fip.fip_periodogram(posteriors, pky, nua, nub, device=0), nu)
    print("p(k | y), merged:        " + "  ".join(f"{p:.4g} +/- {e:.2g} (shrinkage alone {e2:.2g})"
                                                    for p, e, e2 in zip(boot["pky"], boot["pky_err"], shrink["pky_err"])))
    print("p(k | y), median ln Z:   " + "  ".join(f"{p:.4g}" for p in pky))
    print("ln Z, merged:            " + "  ".join(f"{z:.3f} +/- {e:.3f} ({e2:.3f})"
                                                    for z, e, e2 in zip(boot["logz"], boot["logz_err"], shrink["logz_err"])))
    print("ln Z over the runs:      " + "  ".join(f"median {np.median(logzs[:, k]):.3f} std {np.std(logzs[:, k]):.3f}"
                                                    for k in range(3)))
    print(f"lowest log10 FIP, merged: {boot['log10fip'][best]:.3f} +/- {boot['log10fip_err'][best]:.3f} (shrinkage alone "
          f"{shrink['log10fip_err'][best]:.3f}; replicates {boot['log10fip_min'][best]:.3f} .. {boot['log10fip_max'][best]:.3f}) at "
          f"P = {boot['periods'][best]:.4f} d")
    print(f"the per-run curves there: median {s['median'][best]:.3f}, std over {R} runs {s['std'][best]:.3f}; their own lowest "
          f"median {s['median'].min():.3f} at P = {s['periods'][int(np.argmin(s['median']))]:.4f} d; converged: {s['converged']}")
    print(f"median log10 FIP error over the bins: bootstrap {np.median(boot['log10fip_err']):.2e}, shrinkage alone "
          f"{np.median(shrink['log10fip_err']):.2e}, per-run std {np.median(s['std']):.2e}", flush=True)


if __name__ == "__main__":
    flags = ("--gpu-only", "--kernels-only")
    args = [a for a in sys.argv[1:] if a not in flags]
    main(int(args[0]) if args else 128, "--gpu-only" in sys.argv[1:], "--kernels-only" in sys.argv[1:])
