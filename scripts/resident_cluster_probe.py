#!/usr/bin/env python3
"""Clustering inside the resident ensemble (rvll_live_runs_step_clustered) against the three other ways of running R
independent nested-sampling runs of the 51 Peg example (examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points,
dlogz 0.5), for R = 32 and 128 (or the R given):
    host clustered       run_nested_ensemble(walker_runs=model.slice_walk_runs, clustering=True, clusterer=model.cluster_runs)
    resident clustered   run_nested_ensemble(live=model, clustering=True)
    resident unclustered run_nested_ensemble(live=model)
    host unclustered     run_nested_ensemble(walker_runs=model.slice_walk_runs)
Per setting: ln Z median and standard deviation over the runs, likelihood calls, wall time; for the resident clustered ensemble
also the step's time split, summed over its steps — host seconds between the step's synchronisations (GpuRVModel.
live_runs_cluster_phases): clustering + label sort, per-cluster moments, walk — and the cluster counts seen.  Run on the GPU box:
    python3 scripts/resident_cluster_probe.py [R ...]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402


class _Phases:
    """The model, with the phase split of every clustered step added up."""

    def __init__(self, m):
        self.m = m
        self.total = {"cluster_s": 0.0, "moments_s": 0.0, "walk_s": 0.0}
        self.steps = 0

    def __getattr__(self, name):
        return getattr(self.m, name)

    def live_runs_step_clustered(self, *a, **k):
        out = self.m.live_runs_step_clustered(*a, **k)
        for key, v in self.m.live_runs_cluster_phases().items():
            self.total[key] += v
        self.steps += 1
        return out


def main(rs):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            prior, loglike = make_ultranest_callbacks(m, vectorized=True)
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            host = dict(walker_runs=m.slice_walk_runs)
            # warm-up: kernels loaded, buffers sized
            run_nested_ensemble(prior, loglike, m.ndim, [999, 998], clustering=True, clusterer=m.cluster_runs, **host, **kw)
            run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, clustering=True, **kw)
            for R in rs:
                seeds = list(range(1, R + 1))
                print(f"51 Peg, k = {k}, ndim {m.ndim}, nlive 400, dlogz 0.5, R = {R} runs", flush=True)
                walls = {}
                for name in ("host clustered", "resident clustered", "resident unclustered", "host unclustered"):
                    live = _Phases(m) if name == "resident clustered" else m
                    args = dict(kw, clustering=name.endswith(" clustered"))
                    if name.startswith("host"):
                        args.update(host, clusterer=m.cluster_runs if args["clustering"] else None)
                        p, ll = prior, loglike
                    else:
                        args["live"] = live
                        p = ll = None
                    t0 = time.perf_counter()
                    out = run_nested_ensemble(p, ll, m.ndim, seeds, **args)
                    walls[name] = wall = time.perf_counter() - t0
                    lz = np.array([r.logz for r in out])
                    line = (f"  {name:<21}: ln Z median {np.median(lz):9.3f} std {lz.std():7.3f} (min {lz.min():9.3f} max "
                            f"{lz.max():9.3f}); calls {sum(r.ncall for r in out):>12,}; iterations {min(r.niter for r in out)} .. "
                            f"{max(r.niter for r in out)}; wall {wall:6.2f} s")
                    print(line, flush=True)
                    if name == "resident clustered":
                        t = live.total
                        step = sum(t.values())
                        print(f"    its {live.steps} steps: {1e3 * step / live.steps:.2f} ms a step between its first and last "
                              f"synchronisation — clustering + label sort {1e3 * t['cluster_s'] / live.steps:.2f} ms, "
                              f"cluster moments {1e3 * t['moments_s'] / live.steps:.2f} ms, walk {1e3 * t['walk_s'] / live.steps:.2f} ms",
                              flush=True)
                        counts = np.bincount(np.concatenate([r.nclusters for r in out]))
                        print("    clusters per run iteration: " + ", ".join(f"{c}: {n}" for c, n in enumerate(counts) if n), flush=True)
                print(f"  wall time, resident clustered / resident unclustered: "
                      f"{walls['resident clustered'] / walls['resident unclustered']:.2f}; resident clustered / host clustered: "
                      f"{walls['resident clustered'] / walls['host clustered']:.2f}", flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [32, 128])
