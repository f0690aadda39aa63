#!/usr/bin/env python3
"""What a mixed step-count table costs the run-mode walk: R runs of kbatch walkers of the 51 Peg example (k = 1),
walked by GpuRVModel.slice_walk_runs with every run at nsteps = 3 ndim (a uniform table: the rounds form at 6144 .. 24576
walkers) and with the same table but one run a step longer (a mixed table: the single-kernel forms).  Prints likelihood calls
per second inside the walk, best of 5 calls each, alternated.  Run on the GPU box:
    python3 scripts/mixed_table_probe.py [R kbatch]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402


def main(R, kb):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        rng = np.random.default_rng(1)
        cube = rng.random((R * kb * 3, m.ndim))
        theta, logl = m.prior_loglike_batch(cube)
        lstar = float(np.quantile(logl, 0.6))
        keep = logl > lstar
        cube, theta, logl = cube[keep][:R * kb], theta[keep][:R * kb], logl[keep][:R * kb]
        d0 = cube - cube.mean(axis=0)
        chol = np.linalg.cholesky(d0.T @ d0 / (len(cube) - 1) + 1e-14 * np.eye(m.ndim))
        run_start = np.arange(R + 1) * kb
        n = 3 * m.ndim
        tables = {"uniform": np.full(R, n), "mixed": np.concatenate([[n + 1], np.full(R - 1, n)])}
        best = {k: 0.0 for k in tables}
        form = {}
        for _ in range(5):
            for name, steps in tables.items():
                t0 = time.perf_counter()
                _, _, _, nc = m.slice_walk_runs(cube, theta, logl, run_start, np.full(R, lstar), np.repeat(chol[None], R, 0),
                                                wrapped_params(m.parnames), nsteps=steps, seeds=list(range(R)))
                dt = time.perf_counter() - t0
                best[name] = max(best[name], float(np.sum(nc)) / dt)
                form[name] = "rounds" if m.slice_walk_rounds() > 0 else "single kernel"
        print(f"R = {R}, kbatch = {kb}, {R * kb} walkers, nsteps {n}")
        for name in tables:
            print(f"  {name:>8} table ({form[name]}): {best[name]:.3e} calls/s")
        print(f"  mixed / uniform: {best['mixed'] / best['uniform']:.3f}")


if __name__ == "__main__":
    a = [int(x) for x in sys.argv[1:]]
    main(*(a or [128, 100]))
