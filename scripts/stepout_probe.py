#!/usr/bin/env python3
"""Does PolyChord's stepping-out proposal (proposal="stepout") pass the insertion-index test on the 51 Peg
resident ensembles, and at what cost against the chord walk (and, by profiles/adaptive_probe.txt, against the move-distance
adaptation)?  R independent clustered resident runs of examples/51peg/config_51peg.py (k = 1 and 2 planets, 400 live points,
kbatch 100, dlogz 0.5): the chord walk at nsteps = 3 ndim, stepout at 5 ndim (PolyChord's num_repeats) and at 3 ndim, width 1.
Per setting, in the columns of adaptive_probe.txt:
    lnZ sd / iqr     the spread of ln Z over the runs
    fail             runs that fail insertion.test(device=0) at alpha = 0.01; deaths: the median deaths before the first failing window
    shrink           the mean simulated-shrinkage ln Z error (shrinkage.logz_error, device=0)
    calls, wall      likelihood calls over all runs, and the ensemble's wall time
    calls/move       the walks' calls (all calls but the initial live points) per move made
Then the likelihood calls per second inside ONE walk of 16384 walkers at cfg3 (bench.py's workload, nsteps 3 ndim): the chord walk
in its default form against the stepout walk (single kernel), best of 5 alternated calls each.
--kernel-only R k: one stepout clustered ensemble and nothing else (the run to put under rocprofv3 --kernel-trace --stats).
Run on the GPU box:
    python3 scripts/stepout_probe.py [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, insertion, run_nested_ensemble, shrinkage  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402
from evidence_amd.synthetic import make_workload  # noqa: E402

ALPHA = 0.01
CFG = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"


def _model(k):
    rundict, datadict, priordict, fixed = read_config(CFG, nplanets=k)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def ensembles(R):
    print(f"51 Peg resident ensembles, clustered, R = {R}, 400 live points, kbatch 100; insertion test alpha = {ALPHA}", flush=True)
    print(f"{'k':>2} {'proposal':>8} {'nsteps':>6} {'lnZ sd':>7} {'lnZ iqr':>7} {'fail':>5} {'deaths':>7} {'shrink':>7} {'calls':>11} "
          f"{'calls/move':>10} {'wall':>7}", flush=True)
    for k in (1, 2):
        with _model(k) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=200_000_000, clustering=True)
            run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, **kw)                        # kernels loaded
            run_nested_ensemble(None, None, m.ndim, [999, 998], live=m, proposal="stepout", **kw)
            for proposal, mult in (("chord", 3), ("stepout", 5), ("stepout", 3)):
                nsteps = mult * m.ndim
                t0 = time.perf_counter()
                got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, nsteps=nsteps, proposal=proposal,
                                          step_width=1.0, **kw)
                wall = time.perf_counter() - t0
                logz = np.array([g.logz for g in got])
                recs = insertion.test(got, device=0, alpha=ALPHA)["runs"]
                fail = [r for r in recs if r["failed"]]
                deaths = [r["first_window_deaths"] for r in fail if r["first_window_deaths"] is not None]
                err = shrinkage.logz_error(got, device=0)
                calls = sum(g.ncall for g in got)
                moves = sum(g.niter * nsteps for g in got)
                print(f"{k:>2} {proposal:>8} {nsteps:>6} {np.std(logz):>7.2f} {np.subtract(*np.percentile(logz, [75, 25])):>7.2f} "
                      f"{len(fail):>5} {np.median(deaths) if deaths else float('nan'):>7.0f} {np.mean(err):>7.2f} {calls:>11} "
                      f"{(calls - R * 400) / moves:>10.2f} {wall:>6.1f}s", flush=True)


def walk_rate(k_walkers=16384, reps=5):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        rng = np.random.default_rng(1)
        cube = rng.random((3 * k_walkers, m.ndim))
        theta, logl = m.prior_loglike_batch(cube)
        lstar = float(np.quantile(logl, 0.6))
        keep = logl > lstar
        cube, theta, logl = cube[keep][:k_walkers], theta[keep][:k_walkers], logl[keep][:k_walkers]
        d0 = cube - cube.mean(axis=0)
        chol = np.linalg.cholesky(d0.T @ d0 / (len(cube) - 1) + 1e-14 * np.eye(m.ndim))
        wr = wrapped_params(m.parnames)
        n = 3 * m.ndim
        best, form, calls = {}, {}, {}
        for _ in range(reps):
            for proposal in ("chord", "stepout"):
                t0 = time.perf_counter()
                _, _, _, nc = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=n, seed=3, proposal=proposal)
                dt = time.perf_counter() - t0
                best[proposal] = max(best.get(proposal, 0.0), nc / dt)
                calls[proposal] = nc
                form[proposal] = "rounds" if m.slice_walk_rounds() > 0 else "single kernel"
        print(f"cfg3, {len(cube)} walkers, nsteps {n} (3 ndim), one walk; best of {reps}", flush=True)
        for p in best:
            print(f"  {p:>8} ({form[p]}): {best[p]:.3e} calls/s, {calls[p] / (len(cube) * n):.2f} calls/move", flush=True)
        print(f"  stepout / chord: {best['stepout'] / best['chord']:.3f} (calls/s)", flush=True)


def kernel_only(R, k):
    with _model(k) as m:
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=200_000_000, clustering=True)
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, nsteps=5 * m.ndim, proposal="stepout", **kw)
        print(f"k = {k}, R = {R}: {sum(g.ncall for g in got)} calls", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--kernel-only"]:
        kernel_only(int(sys.argv[2]), int(sys.argv[3]))
    else:
        ensembles(int(sys.argv[1]) if len(sys.argv) > 1 else 128)
        walk_rate()
