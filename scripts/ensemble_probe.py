#!/usr/bin/env python3
"""Wall time of R independent nested-sampling runs of the 51 Peg example (examples/51peg/config_51peg.py, one planet,
400 live points) back to back — run_nested_slice(walker=model.slice_walk), one run after the other — against the same R
seeds through run_nested_ensemble(walker_runs=model.slice_walk_runs), where one device walk per iteration carries the
walkers of every run still going.  Checks that both give the same ln Z, iterations and calls for every seed, and splits the
ensemble's wall time into the walk calls and the host's per-run bookkeeping.  Run on the GPU box:
    python3 scripts/ensemble_probe.py [R ...]          (default 1 8 32 128)"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402
from evidence_amd.nested import run_nested_slice  # noqa: E402

rs = [int(a) for a in sys.argv[1:]] or [1, 8, 32, 128]
cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
    prior, loglike = make_ultranest_callbacks(m, vectorized=True)
    kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=20_000_000)
    print(f"51 Peg, 1 planet, ndim {m.ndim}, nlive 400 (kbatch 100, nsteps {3 * m.ndim}), dlogz 0.5")
    run_nested_slice(prior, loglike, m.ndim, seed=999, walker=m.slice_walk, **kw)           # warm-up: kernels loaded, buffers sized
    run_nested_ensemble(prior, loglike, m.ndim, [998, 997], walker_runs=m.slice_walk_runs, **kw)
    print(f"{'R':>4} {'back to back s':>15} {'ensemble s':>11} {'speed-up':>9} {'walk calls':>10} {'walk s':>8} {'host s':>8} "
          f"{'host share':>10} {'ms/turn walk':>12} {'ms/turn host':>12} {'walkers/turn':>12} {'same lnZ':>8}")
    for R in rs:
        seeds = list(range(1, R + 1))
        t0 = time.perf_counter()
        alone = [run_nested_slice(prior, loglike, m.ndim, seed=s, walker=m.slice_walk, **kw) for s in seeds]
        t_alone = time.perf_counter() - t0
        walk = {"s": 0.0, "n": 0, "rows": 0}

        def walker_runs(*a, **k):
            t = time.perf_counter()
            out = m.slice_walk_runs(*a, **k)
            walk["s"] += time.perf_counter() - t
            walk["n"] += 1
            walk["rows"] += len(a[0])
            return out

        t0 = time.perf_counter()
        ens = run_nested_ensemble(prior, loglike, m.ndim, seeds, walker_runs=walker_runs, **kw)
        t_ens = time.perf_counter() - t0
        same = all(e.logz == a.logz and e.niter == a.niter and e.ncall == a.ncall for e, a in zip(ens, alone))
        host = t_ens - walk["s"]
        print(f"{R:>4} {t_alone:>15.2f} {t_ens:>11.2f} {t_alone / t_ens:>9.2f} {walk['n']:>10} {walk['s']:>8.2f} {host:>8.2f} "
              f"{host / t_ens:>10.2f} {1e3 * walk['s'] / walk['n']:>12.2f} {1e3 * host / walk['n']:>12.2f} "
              f"{walk['rows'] / walk['n']:>12.0f} {str(same):>8}", flush=True)
        lz = np.array([e.logz for e in ens])
        print(f"     ln Z over the {R} runs: median {np.median(lz):.3f}, std {lz.std():.3f}; iterations {min(e.niter for e in ens)} .. "
              f"{max(e.niter for e in ens)}; likelihood calls {sum(e.ncall for e in ens):,}", flush=True)
