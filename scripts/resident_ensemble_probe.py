#!/usr/bin/env python3
"""Wall time of R independent nested-sampling runs of the 51 Peg example (examples/51peg/config_51peg.py, one planet, 400 live
points) through run_nested_ensemble in its two forms: the host ensemble (walker_runs=model.slice_walk_runs: per-run
bookkeeping on the host, one shared walk per iteration) and the resident ensemble (live=model: every run's live set in HBM,
one sort call and one step call per iteration).  Checks that the resident ensemble's ln Z, iterations and calls equal those
of the standalone resident runs run_nested_slice(live=model) seed by seed, and splits its wall time per turn into the step
call and the host (sort call, draws, evidence sums).  Run on the GPU box:
    python3 scripts/resident_ensemble_probe.py [R ...]          (default 1 8 32 128)
    python3 scripts/resident_ensemble_probe.py --resident-only R   (one resident ensemble, for a profiler run)"""
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

args = sys.argv[1:]
resident_only = bool(args) and args[0] == "--resident-only"
rs = [int(a) for a in (args[1:] if resident_only else args)] or [1, 8, 32, 128]
cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
    prior, loglike = make_ultranest_callbacks(m, vectorized=True)
    kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=20_000_000)
    print(f"51 Peg, 1 planet, ndim {m.ndim}, nlive 400 (kbatch 100, nsteps {3 * m.ndim}), dlogz 0.5")
    run_nested_ensemble(None, None, m.ndim, [998, 997], live=m, **kw)        # warm-up: kernels loaded, buffers sized
    if resident_only:
        for R in rs:
            t0 = time.perf_counter()
            ens = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, **kw)
            print(f"R {R}: resident ensemble {time.perf_counter() - t0:.2f} s, {ens[0].timing['turns']} turns of run 1", flush=True)
        sys.exit(0)
    run_nested_slice(None, None, m.ndim, seed=999, live=m, **kw)
    run_nested_ensemble(prior, loglike, m.ndim, [998, 997], walker_runs=m.slice_walk_runs, **kw)
    print(f"{'R':>4} {'host ens s':>10} {'resident s':>10} {'vs host':>8} {'turns':>6} {'step s':>7} {'host s':>7} {'host share':>10} "
          f"{'ms/turn step':>12} {'ms/turn host':>12} {'alone s':>8} {'same as alone':>13}")
    for R in rs:
        seeds = list(range(1, R + 1))
        t0 = time.perf_counter()
        hens = run_nested_ensemble(prior, loglike, m.ndim, seeds, walker_runs=m.slice_walk_runs, **kw)
        t_host = time.perf_counter() - t0
        t0 = time.perf_counter()
        ens = run_nested_ensemble(None, None, m.ndim, seeds, live=m, **kw)
        t_res = time.perf_counter() - t0
        t0 = time.perf_counter()
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **kw) for s in seeds]
        t_alone = time.perf_counter() - t0
        same = all(e.logz == a.logz and e.niter == a.niter and e.ncall == a.ncall for e, a in zip(ens, alone))
        turns = max(e.timing["turns"] for e in ens)
        step = max(e.timing["walk_s"] for e in ens)            # every step call is counted in full by the runs that took part
        host = t_res - step
        print(f"{R:>4} {t_host:>10.2f} {t_res:>10.2f} {t_res / t_host:>8.2f} {turns:>6} {step:>7.2f} {host:>7.2f} {host / t_res:>10.2f} "
              f"{1e3 * step / turns:>12.2f} {1e3 * host / turns:>12.2f} {t_alone:>8.2f} {str(same):>13}", flush=True)
        lz = np.array([e.logz for e in ens])
        print(f"     ln Z over the {R} runs: median {np.median(lz):.3f}, std {lz.std():.3f}; iterations {min(e.niter for e in ens)} .. "
              f"{max(e.niter for e in ens)}; likelihood calls {sum(e.ncall for e in ens):,} (host ensemble: median ln Z "
              f"{np.median([e.logz for e in hens]):.3f})", flush=True)
