#!/usr/bin/env python3
"""The correlated-noise likelihood at the cfg3 shape: B = 16384 parameter vectors x 200 epochs of the synthetic
workload 3, with one noise term of J = 1 (real), 2 (sho) and 4 (rotation) columns whose parameters are free, and the last two
again with Q within 0.005 of 1/2, where the solve carries the SHO's two columns in the pair basis.
    device      correlated.CorrelatedNoiseModel.log_likelihood_batch after a warm-up call: HIP-event time of the residual stage
                (launch_residuals: keprv_kernel + residual_kernel) and of the solve (celerite_kernel<J>), and rows/s of the whole
                call with its upload and download, best of REPEATS calls
    white       GpuRVModel.log_likelihood_batch on the same rows, best of REPEATS calls, and the white kernel's own time
                (dev_time_loglike), for scale
    definition  correlated.log_likelihood_dense (numpy Cholesky) on residuals_batch of DENSE_ROWS of the rows, scaled to B
                (labelled as scaled), and the largest |device - definition| / max(1, |definition|) over those rows
Run on the GPU box:  python3 scripts/celerite_probe.py [B [output]]; the text goes to profiles/celerite_probe.txt unless an output
path is given."""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, correlated  # noqa: E402
from evidence_amd.synthetic import make_workload  # noqa: E402

REPEATS = 5
DENSE_ROWS = 64
TERMS = [(1, "real", {"gp1_sigma": (1.0, 3.0), "gp1_tau": (5.0, 50.0)}),
         (2, "sho", {"gp1_sigma": (1.0, 3.0), "gp1_rho": (5.0, 50.0), "gp1_q": (0.6, 5.0)}),
         (4, "rotation", {"gp1_sigma": (1.0, 3.0), "gp1_prot": (5.0, 50.0), "gp1_q0": (0.5, 3.0), "gp1_dq": (0.1, 2.0),
                          "gp1_mix": (0.1, 1.0)}),
         # every row in the pair basis of csrc/rvll_celerite.h (|q - 1/2| < 0.01), on both sides of 1/2; the rotation's faster oscillator
         (2, "sho", {"gp1_sigma": (1.0, 3.0), "gp1_rho": (5.0, 50.0), "gp1_q": (0.495, 0.505)}),
         (4, "rotation", {"gp1_sigma": (1.0, 3.0), "gp1_prot": (5.0, 50.0), "gp1_q0": (1e-6, 5e-3), "gp1_dq": (0.1, 2.0),
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
    say(f"cfg3 shape: B = {B} rows x {w.table.n_epochs} epochs, {w.ndim} model parameters; times are the best of {REPEATS} calls "
        f"after a warm-up call")
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        m.log_likelihood_batch(base)
        white_s = best(lambda: m.log_likelihood_batch(base))
        m.dev_upload_theta(base)
        kt = m.dev_time_loglike(B)
        say(f"  white (GpuRVModel.log_likelihood_batch):  call {1e3 * white_s:8.3f} ms = {B / white_s:.3e} rows/s   kernel "
            f"{kt['kernel_ms_median']:8.3f} ms (median of {kt['launches']})")
    worst_all = 0.0
    for J, kind, ranges in TERMS:
        names = sorted(w.parnames + list(ranges))
        X = np.empty((B, len(names)))
        for j, n in enumerate(names):
            X[:, j] = rng.uniform(*ranges[n], B) if n in ranges else base[:, w.parnames.index(n)]
        with GpuRVModel(w.fixedpardict, w.table, names) as m:
            gp = correlated.CorrelatedNoiseModel(m, [(kind, "gp1")])
            gp.log_likelihood_batch(X)
            t = {}
            got, flags = gp.log_likelihood_batch(X, return_flags=True, timing=t)
            call_s = best(lambda: gp.log_likelihood_batch(X))
            rows = X[:DENSE_ROWS]
            res, var = m.residuals_batch(rows)
            t0 = time.perf_counter()
            want = np.array([correlated.log_likelihood_dense(res[i], var[i], m.table.time, gp.columns(rows[i]))
                             for i in range(DENSE_ROWS)])
            dense_s = (time.perf_counter() - t0) * B / DENSE_ROWS
            ok = (flags[:DENSE_ROWS] == 0) & (want > -1e29)
            worst = float(np.max(np.abs(got[:DENSE_ROWS] - want)[ok] / np.maximum(1.0, np.abs(want[ok]))))
            worst_all = max(worst_all, worst)
            pair = " near 1/2" if any(n.endswith(("_q", "_q0")) and hi < 0.51 for n, (_, hi) in ranges.items()) else ""
            say(f"  J = {J} ({kind:8s}{pair}):  residual stage {t['residuals_ms']:8.3f} ms   solve {t['solve_ms']:8.3f} ms   call "
                f"{1e3 * call_s:8.3f} ms = {B / call_s:.3e} rows/s   flagged rows {int((flags != 0).sum())}")
            say(f"      definition (numpy Cholesky, scaled from {DENSE_ROWS} rows x {B // DENSE_ROWS}): {dense_s:8.2f} s = "
                f"{B / dense_s:.3e} rows/s   call / definition {call_s / dense_s:.2e}   largest |device - definition| / "
                f"max(1, |definition|) over {int(ok.sum())} rows: {worst:.3e}")
    say(f"largest relative difference to the definition in this run: {worst_all:.3e}")


if __name__ == "__main__":
    args = sys.argv[1:]
    path = Path(args[1]) if len(args) > 1 else Path(__file__).resolve().parents[1] / "profiles" / "celerite_probe.txt"
    with open(path, "w") as fh:
        main(int(args[0]) if args else 16384, fh)
