#!/usr/bin/env python3
"""MLFriends region sampling against the chord walk on the same runs and the same card.  R = 32 independent runs
of the 51 Peg example (examples/51peg/config_51peg.py, k = 0 and 1 planets, 400 live points, kbatch 100, dlogz 0.5) through the
host-managed ensemble (run_nested_ensemble), once with proposal="region" (region_runs = GpuRVModel.region_draw_runs, clusterer =
GpuRVModel.cluster_runs, short runs finished by GpuRVModel.slice_walk_runs) and once with the chord walk
(walker_runs = GpuRVModel.slice_walk_runs).  Per setting:
    wall         seconds of the whole ensemble
    calls        likelihood calls, summed over the runs
    fallbacks    points the walk supplied because a region draw stayed short (region only), and the iterations that had any
    efficiency   accepted / calls of the region draw by iteration: the median over runs at every tenth of the run
    ln Z         median and standard deviation over the runs, and the mean simulated-shrinkage error of one run
    pass         the share of runs that pass insertion.test at alpha = 0.01, and the pooled p-value
Writes profiles/region_probe.txt.  Run on the GPU box:
    python3 scripts/region_probe.py [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, insertion, run_nested_ensemble, shrinkage  # noqa: E402
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


def main(R):
    cfg = ROOT / "examples" / "51peg" / "config_51peg.py"
    lines = [f"region sampling against the chord walk: {R} runs of 51 Peg, nlive 400, kbatch 100, dlogz 0.5; ln Z in nats",
             f"{'k':>2} {'proposal':>8} {'wall s':>8} {'calls':>12} {'fallbacks':>10} {'iters w/ fb':>11} {'lnZ median':>11} {'lnZ sd':>7} "
             f"{'shrink err':>10} {'pass':>6} {'pooled p':>9}"]
    effs = []
    for k in (0, 1):
        _rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            prior, loglike = make_ultranest_callbacks(m, vectorized=True)
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000, walker_runs=m.slice_walk_runs)
            settings = {"region": dict(proposal="region", region_runs=m.region_draw_runs, clusterer=m.cluster_runs), "chord": {}}
            run_nested_ensemble(prior, loglike, m.ndim, [999], max_iter=400, **{**kw, **settings["region"]})      # kernels loaded
            for name, extra in settings.items():
                t0 = time.perf_counter()
                got = run_nested_ensemble(prior, loglike, m.ndim, list(range(1, R + 1)), **kw, **extra)
                wall = time.perf_counter() - t0
                logz = np.array([g.logz for g in got])
                err = float(np.mean(shrinkage.logz_error(got, device=0)))
                test = insertion.test(got, device=0)
                passed = np.mean([not rec["failed"] for rec in test["runs"]])
                fb = sum(g.region_fallbacks for g in got) if name == "region" else 0
                fbit = 0
                if name == "region":
                    n_it = max(len(g.region_efficiency) for g in got)
                    eff = np.full((R, n_it), np.nan)
                    for r, g in enumerate(got):
                        eff[r, :len(g.region_efficiency)] = g.region_efficiency
                    fbit = int(np.sum([np.count_nonzero(np.isnan(g.region_efficiency) | (g.region_calls == 0)) for g in got]))
                    with np.errstate(all="ignore"):
                        med = np.nanmedian(eff, axis=0)
                    at = np.linspace(0, n_it - 1, 11).astype(int)
                    effs.append(f"k = {k}: region efficiency (median over runs) at iteration " +
                                ", ".join(f"{i}: {med[i]:.4f}" for i in at))
                lines.append(f"{k:>2} {name:>8} {wall:>8.2f} {sum(g.ncall for g in got):>12d} {fb:>10d} {fbit:>11d} {np.median(logz):>11.3f} "
                             f"{np.std(logz):>7.3f} {err:>10.3f} {passed:>6.2f} {test['pooled']['pvalue']:>9.2e}")
                print(lines[-1], flush=True)
    out = "\n".join(lines + effs) + "\n"
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "region_probe.txt").write_text(out)
    print(out)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
