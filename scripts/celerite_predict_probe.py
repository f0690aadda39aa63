#!/usr/bin/env python3
"""GP prediction under correlated noise at the cfg3 shape: the synthetic workload 3 (200 epochs) with one noise term
of J = 1 (real), 2 (sho) and 4 (rotation) columns whose parameters are free.
    mean        B = 16384 rows, M = 0 and M = 512 query times, without the variance at the query times: the HIP-event times of
                the residual stage, the factor sweep (celerite_kernel<J> with its stores), the backward and forward sweeps, and the whole
                call with its upload, transposes and downloads (best of REPEATS calls after a warm-up call); beside them the
                log-L call on the same rows (its solve, celerite_kernel<J>, and the whole call)
    variance    256 rows x 512 query times with the variance at the query times (cel_gridvar_kernel<J>)
    error       the largest |device - reference| / max(1, |reference|) of every output against the dense definition in long
                double (tests/predict_cases.dense_predict_reference) on REF_ROWS rows and REF_TIMES of the query times
Run on the GPU box:  python3 scripts/celerite_predict_probe.py [B [output]]; the text goes to profiles/celerite_predict_probe.txt
unless an output path is given."""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import numpy as np  # noqa: E402

import correlated_cases as cc  # noqa: E402
import predict_cases as pc  # noqa: E402
from evidence_amd import GpuRVModel, correlated  # noqa: E402
from evidence_amd.synthetic import make_workload  # noqa: E402

REPEATS = 5
M = 512
VAR_ROWS = 256
REF_ROWS = 8
REF_TIMES = 64
TERMS = [(1, "real", {"gp1_sigma": (1.0, 3.0), "gp1_tau": (5.0, 50.0)}),
         (2, "sho", {"gp1_sigma": (1.0, 3.0), "gp1_rho": (5.0, 50.0), "gp1_q": (0.6, 5.0)}),
         (4, "rotation", {"gp1_sigma": (1.0, 3.0), "gp1_prot": (5.0, 50.0), "gp1_q0": (0.5, 3.0), "gp1_dq": (0.1, 2.0),
                          "gp1_mix": (0.1, 1.0)})]


def best(f, n=REPEATS):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        out.append(time.perf_counter() - t0)
    return min(out)


def main(B, out):
    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    w = make_workload(3)
    base = w.sample_theta(B, seed=11)
    rng = np.random.default_rng(12)
    t = np.asarray(w.table.time, dtype=np.float64)
    x = np.sort(rng.uniform(t.min() - 5.0, t.max() + 5.0, M))
    say(f"cfg3 shape: B = {B} rows x {w.table.n_epochs} epochs, {w.ndim} model parameters, M = {M} query times; call times are the "
        f"best of {REPEATS} calls after a warm-up call, phase times the HIP events of one call")
    worst_all = 0.0
    for J, kind, ranges in TERMS:
        names = sorted(w.parnames + list(ranges))
        X = np.empty((B, len(names)))
        for j, n in enumerate(names):
            X[:, j] = rng.uniform(*ranges[n], B) if n in ranges else base[:, w.parnames.index(n)]
        with GpuRVModel(w.fixedpardict, w.table, names) as m:
            gp = correlated.CorrelatedNoiseModel(m, [(kind, "gp1")])
            gp.log_likelihood_batch(X)
            tl = {}
            gp.log_likelihood_batch(X, timing=tl)
            logl_s = best(lambda: gp.log_likelihood_batch(X))
            say(f"  J = {J} ({kind}):")
            say(f"      log-L call          residuals {tl['residuals_ms']:8.3f} ms   solve  {tl['solve_ms']:8.3f} ms"
                f"{'':41s}   call {1e3 * logl_s:8.3f} ms")
            for label, times in (("M = 0  ", None), (f"M = {M}", x)):
                gp.predict_batch(X, times)
                tp = {}
                gp.predict_batch(X, times, timing=tp)
                call_s = best(lambda: gp.predict_batch(X, times))
                say(f"      predict, {label}    residuals {tp['residuals_ms']:8.3f} ms   factor {tp['factor_ms']:8.3f} ms   backward + forward "
                    f"{tp['sweeps_ms']:8.3f} ms   call {1e3 * call_s:8.3f} ms = {B / call_s:.3e} rows/s")
            rows = X[:VAR_ROWS]
            gp.predict_batch(rows, x, return_var=True)
            tv = {}
            got = gp.predict_batch(rows, x, return_var=True, timing=tv)
            var_s = best(lambda: gp.predict_batch(rows, x, return_var=True))
            say(f"      with the variance, {VAR_ROWS} rows x {M} times: factor {tv['factor_ms']:8.3f} ms   backward + forward "
                f"{tv['sweeps_ms']:8.3f} ms   variance {tv['variance_ms']:8.3f} ms   call {1e3 * var_s:8.3f} ms")
            pick = np.linspace(0, M - 1, REF_TIMES).astype(int)
            res, var = m.residuals_batch(rows[:REF_ROWS])
            cols = np.array([gp.columns(r) for r in rows[:REF_ROWS]])
            want = pc.dense_predict_reference(res, var, t, cols, x[pick])
            errs = {"mean_data": cc.ref_err(got.mean_data[:REF_ROWS], want["mean_data"]).max(),
                    "var_data": cc.ref_err(got.var_data[:REF_ROWS], want["var_data"]).max(),
                    "mean": cc.ref_err(got.mean[:REF_ROWS][:, pick], want["mean"]).max(),
                    "var": cc.ref_err(got.var[:REF_ROWS][:, pick], want["var"]).max()}
            assert not got.flags[:REF_ROWS].any()
            worst_all = max(worst_all, max(errs.values()))
            say(f"      largest |device - long double| / max(1, |long double|) over {REF_ROWS} rows, {REF_TIMES} of the times:  "
                + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    say(f"largest error against the long-double reference in this run: {worst_all:.3e}")


if __name__ == "__main__":
    args = sys.argv[1:]
    path = Path(args[1]) if len(args) > 1 else ROOT / "profiles" / "celerite_predict_probe.txt"
    with open(path, "w") as fh:
        main(int(args[0]) if args else 16384, fh)
