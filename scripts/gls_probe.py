#!/usr/bin/env python3
"""Residual GLS periodograms of merged runs: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 0 and 1 planets, 400 live points, dlogz 0.5), S = 1000 replicates with the run bootstrap,
n = 256 draws a replicate, the default grid periodogram.frequency_grid(table.time).
    gls_bands   GpuRVModel.gls_bands on the S x n drawn rows after a warm-up call on 8 replicates: HIP-event time of the residual
                stage, of the periodogram kernel and of the reductions (order statistics and peaks), the wall time of the call with
                its upload and downloads, and the periodogram kernel's share of the fp64 vector peak by operation count — 6 fused
                multiply-adds a (draw, epoch, frequency) term are the useful work; the sincos and the rotation a thread spends on
                an (epoch, frequency pair) are overhead and not counted
    new route   periodogram.residual_gls(device=0) on NEW_REPS replicates, wall
    host route  the route without this code: residuals_batch to the host and periodogram.gls_definition there, timed on HOST_ROWS
                rows x HOST_FREQ frequencies and scaled to S x n rows and the whole grid (labelled as scaled)
Run on the GPU box:  python3 scripts/gls_probe.py [R [output [S]]]; the text goes to profiles/gls_probe.txt unless an output path
is given."""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, draws, periodogram, predictive, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

NDRAWS = 256
NEW_REPS = 100
HOST_ROWS, HOST_FREQ = 16, 8192
LEVELS = predictive.QUANTILES
PEAK_FP64_VECTOR_TFLOPS = 78.6          # MI355X: 256 CUs x 4 SIMDs x 16 lanes x 2 flops x 2.4 GHz


def probe(k, R, S, cfg, say):
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
        ne = m.table.time.shape[0]
        f0, df, nfreq = periodogram.frequency_grid(m.table.time)
        say(f"k = {k}: R = {R} runs, {sum(len(g.logl) for g in got)} merged rows, S = {S} replicates (run bootstrap, random "
            f"shrinkage), n = {NDRAWS} draws a replicate, {ne} epochs, default grid: {nfreq} frequencies from {f0:.3e} to "
            f"{f0 + df * (nfreq - 1):.4f} 1/d; one call after a warm-up call on 8 replicates")
        theta = draws.samples(got, NDRAWS, S, seed=1, device=0)
        alive = ~np.isnan(theta[:, 0, 0])
        theta = np.where(alive[:, None, None], theta, theta[int(np.argmax(alive))][None])
        m.gls_bands(theta[:8], f0, df, nfreq, LEVELS)
        t = {}
        t0 = time.perf_counter()
        out = m.gls_bands(theta, f0, df, nfreq, LEVELS, timing=t)
        wall = time.perf_counter() - t0
        terms = float(S) * NDRAWS * ne * nfreq
        tflops = 12.0 * terms / (1e-3 * t["gls_ms"]) / 1e12
        say(f"  gls_bands (rvll_gls_bands):  residuals {t['residuals_ms']:9.2f} ms   periodogram {t['gls_ms']:10.2f} ms   reductions "
            f"{t['reduce_ms']:10.2f} ms   call {wall:8.2f} s   for {terms:.3g} (draw, epoch, frequency) terms")
        say(f"      periodogram kernel: {1e9 * t['gls_ms'] / terms:.4f} ps a term; 6 FMA a term = {tflops:.1f} TFLOP/s, "
            f"{100.0 * tflops / PEAK_FP64_VECTOR_TFLOPS:.1f} % of the {PEAK_FP64_VECTOR_TFLOPS} TFLOP/s fp64 vector peak")
        median = out["q"][:, 1, :][alive].mean(axis=0)
        top = int(np.argmax(median))
        say(f"      the median band's top: power {float(median[top]):.4f} at P = "
            f"{1.0 / (f0 + df * top):.4f} d")
        del out

        reps = min(NEW_REPS, S)
        t0 = time.perf_counter()
        new = periodogram.residual_gls(got, m, ndraws=NDRAWS, nsamples=reps, seed=1, device=0)
        new_s = time.perf_counter() - t0
        top = int(np.argmax(new["band"][1]))
        say(f"  new route (periodogram.residual_gls, device=0, {reps} replicates):  wall {new_s:8.2f} s   median band's top "
            f"{new['band'][1][top]:.4f} +/- {new['band_err'][1][top]:.4f} at P = {new['period'][top]:.4f} d, peak_fraction there "
            f"{new['peak_fraction'][top]:.3f} +/- {new['peak_fraction_err'][top]:.3f}")

        rows = theta.reshape(-1, theta.shape[2])[:HOST_ROWS]
        nf = min(HOST_FREQ, nfreq)
        t0 = time.perf_counter()
        res, var = m.residuals_batch(rows)
        periodogram.gls_definition(m.table.time, res, var, f0, df, nf)
        host_s = (time.perf_counter() - t0) * (float(S) * NDRAWS / HOST_ROWS) * (nfreq / nf)
        say(f"  host route (residuals_batch, gls_definition in numpy):  wall {host_s:10.0f} s = {host_s / 3600.0:.1f} h, scaled from "
            f"{HOST_ROWS} rows x {nf} frequencies (x {S * NDRAWS // HOST_ROWS} x {nfreq / nf:.1f})")
        say(f"  gls_bands call / host route: {wall / host_s:.2e}")
        say()


def main(R, S, out):
    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (0, 1):
        probe(k, R, S, cfg, say)


if __name__ == "__main__":
    args = sys.argv[1:]
    path = Path(args[1]) if len(args) > 1 else Path(__file__).resolve().parents[1] / "profiles" / "gls_probe.txt"
    with open(path, "w") as fh:
        main(int(args[0]) if args else 128, int(args[2]) if len(args) > 2 else 1000, fh)
