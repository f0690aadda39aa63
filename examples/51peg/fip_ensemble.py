#!/usr/bin/env python3
"""The reference's FIP workflow (evidence/fip_criterion.py) end to end on one GPU, for the 51 Peg example: for k = 0, 1, 2
planets, R independent nested-sampling runs through nested.run_nested_ensemble (their walks in one device walk per
iteration), then p(k | y) from the median ln Z over the runs (fip.model_probabilities) and the FIP periodogram of every run
(fip.fip_periodogram); and last the parameter table of the k = 1 model from its R runs merged by their birth contours, every entry
with the scatter over bootstrap replicates of the runs as its error (posterior.table), and the FIP periodogram of the merged runs
of every model with the same scatter as the error of log10 FIP and of p(k | y) (fip.merged_fip), and the period marginal of the k = 1 model with
the same scatter as the error of every bin (marginals.marginals).  Needs a GPU.
    python3 examples/51peg/fip_ensemble.py [R]          (default 8 runs per model)"""
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
from evidence_amd import GpuRVModel, fip, marginals, posterior, run_nested_ensemble      # noqa: E402
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params   # noqa: E402
from evidence_amd.config import read_config                        # noqa: E402

R = int(sys.argv[1]) if len(sys.argv) > 1 else 8
cfg = Path(__file__).with_name("config_51peg.py")
seeds = list(range(1, R + 1))
logzs = np.empty((R, 3))
posteriors = [[None] * 3 for _ in range(R)]              # posteriors[r][k] = (periods [n, k], weights [n]), k >= 1
per_model, period_columns = [], []                       # the runs of every k and the sample columns of its periods
for k in range(3):
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        t0 = time.perf_counter()
        res = run_nested_ensemble(prior, loglike, m.ndim, seeds, nlive=25 * m.ndim, dlogz=0.5, max_calls=50_000_000,
                                  wrapped=wrapped_params(m.parnames), walker_runs=m.slice_walk_runs)
        dt = time.perf_counter() - t0
        cols = [m.parnames.index(f"planet{j}_period") for j in range(1, k + 1)]
        per_model.append(res)
        period_columns.append(cols)
        for r, out in enumerate(res):
            logzs[r, k] = out.logz
            if k:
                posteriors[r][k] = (out.samples[:, cols], np.exp(out.logwt))
        if k == 1:
            one_planet, one_planet_names = res, list(m.parnames)
    print(f"{rundict['target']}, {k} planet(s), {R} runs in {dt:.2f} s: ln Z median {np.median(logzs[:, k]):.3f}, "
          f"std {np.std(logzs[:, k]):.3f}")

pky = fip.model_probabilities(logzs)
print("p(k | y) for k = 0, 1, 2:", " ".join(f"{p:.4g}" for p in pky))
tobs = fip.observation_span(datadict)
nu, nua, nub = fip.frequency_grid(1.5, 1000.0, tobs)
fapnu = fip.fip_periodogram(posteriors, pky, nua, nub, device=0)
s = fip.fip_summary(fapnu, nu)
best = int(np.argmin(s["median"]))
print(f"FIP periodogram over {R} runs, {nu.size} frequencies: lowest median log10 FIP {s['median'][best]:.2f} at "
      f"P = {s['periods'][best]:.4f} d; converged across runs: {s['converged']}")

# the k = 1 model's parameters from its merged runs: point estimates, and the scatter over 1000 bootstrap replicates as errors
print(f"\n1 planet, {R} runs merged:")
print(posterior.format_table(posterior.table(one_planet, one_planet_names, nsamples=1000, seed=1, device=0)))

# the periodogram of the merged runs of every model: every replicate has its own p(k | y) from its own ln Z
mf = fip.merged_fip(per_model, period_columns, nua, nub, nsamples=1000, seed=1, device=0, nu=nu)
best = int(np.argmin(mf["log10fip"]))
print(f"\nFIP periodogram of the merged runs, 1000 bootstrap replicates: lowest log10 FIP {mf['log10fip'][best]:.2f} +/- "
      f"{mf['log10fip_err'][best]:.2f} at P = {mf['periods'][best]:.4f} d")
print("p(k | y) for k = 0, 1, 2:", " ".join(f"{p:.4g} +/- {e:.2g}" for p, e in zip(mf["pky"], mf["pky_err"])))

# the period marginal of the k = 1 model from its merged runs: the density of every bin with its scatter over the replicates
mg = marginals.marginals(one_planet, one_planet_names, columns=["planet1_period"], bins=20, corner=False, nsamples=1000, seed=1,
                         device=0)["panels"][0]
print("\nplanet1_period marginal (density per day, +/- over 1000 bootstrap replicates, min .. max):")
for lo, hi, d, e, a, b in zip(mg["edges"][0][:-1], mg["edges"][0][1:], mg["density"], mg["density_err"], mg["density_min"],
                              mg["density_max"]):
    print(f"  [{lo:.6f}, {hi:.6f})  {d:10.1f} +/- {e:8.1f}   {a:10.1f} .. {b:10.1f}")
