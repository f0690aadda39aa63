#!/usr/bin/env python3
"""Prior sensitivity of ln Z and p(k | y) from merged runs: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 0, 1 and 2 planets, 400 live points, dlogz 0.5), reweighted to A = 64 alternative priors —
the upper bound of every planet's K from 60 to 100 m/s in 32 steps (the base is Jeffreys(0.1, 100)), each with the period prior
left uniform in frequency and changed to Jeffreys(1, 100) — over S = 1000 replicates with the run bootstrap, with no new sampling.
Per k, medians of REPEATS calls after a warm-up call:
    table      sensitivity.log_ratios(device=0): two calls of rvll_prior_logpdf_batch (base and alternative sets over the
               overridden parameters) — HIP-event time of the kernels, the C calls and the wall time of the Python call; the
               rate is densities (rows x sets x parameters, SKIP entries included) a second of kernel time
    numpy      the same table from priors.log_density (device=None), timed on NUMPY_ROWS rows and scaled to N (labelled)
    reweight   sensitivity.reweight_arrays(device=0): the table through rvll_pointwise_replicates, its parts as
               scripts/pointwise_probe.py prints them
then per alternative ln Z' - ln Z with its error over the replicates, efficiency and outside for the models with planets, and
p(k | y) under the base prior and under the five alternatives that move p(1 | y) most.
Run on the GPU box:  python3 scripts/sensitivity_probe.py [--gpu-only] [R]"""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, fip, pointwise, priors, run_nested_ensemble, sensitivity  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
REPEATS = 3
NUMPY_ROWS = 100_000
KMAX = np.geomspace(60.0, 100.0, 32)                  # 51 Peg b has K = 56 m/s: a bound below it leaves no row with weight
MAX_PLANETS = 2


def alternatives():
    """64 dicts that name the K and period priors of every planet up to MAX_PLANETS; a model applies those it has."""
    out, labels = [], []
    for family in ("UniformFrequency", "Jeffreys"):
        for kmax in KMAX:
            alt = {}
            for j in range(1, MAX_PLANETS + 1):
                alt[f"planet{j}_k1"] = priors.Jeffreys(0.1, float(kmax))
                if family == "Jeffreys":
                    alt[f"planet{j}_period"] = priors.Jeffreys(1.0, 100.0)
            out.append(alt)
            labels.append(f"K < {kmax:6.2f}, period {family}")
    return out, labels


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def probe(k, samples, logl, birth, run_start, parnames, priordict, alts, gpu_only):
    n = logl.size
    kw = dict(device=0, skip_missing=True)
    sensitivity.log_ratios(samples, parnames, priordict, alts, **kw)                    # warm-up at the timed shape
    rows, wall = [], []
    for _ in range(REPEATS):
        t = {}
        t0 = time.perf_counter()
        ratio = sensitivity.log_ratios(samples, parnames, priordict, alts, timing=t, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        rows.append(t)
    kern = med(rows, "kernel_ms")
    print(f"  table (2 x rvll_prior_logpdf_batch, {len(alts)} sets of {len(parnames)} parameters, {rows[0]['launches']} launches): "
          f"kernels {kern:.2f} ms ({min(r['kernel_ms'] for r in rows):.2f} .. {max(r['kernel_ms'] for r in rows):.2f}) = "
          f"{rows[0]['elements'] / (kern * 1e-3):.3e} densities/s; C calls {med(rows, 'total_ms'):.1f} ms; Python call "
          f"{float(np.median(wall)):.1f} ms", flush=True)
    if not gpu_only:
        sub = samples[:NUMPY_ROWS]
        t0 = time.perf_counter()
        ref = sensitivity.log_ratios(sub, parnames, priordict, alts, skip_missing=True)
        numpy_s = (time.perf_counter() - t0) * n / sub.shape[0]
        f = np.isfinite(ref)
        same = np.array_equal(np.isneginf(ref), np.isneginf(ratio[:sub.shape[0]]))
        err = float(np.max(np.abs(ref[f] - ratio[:sub.shape[0]][f]))) if same else float("nan")
        print(f"  numpy definition: {numpy_s:.1f} s scaled from {sub.shape[0]} rows (x {n / sub.shape[0]:.1f}); device against it "
              f"there: the same rows excluded: {same}, max |ln r err| {err:.1e}", flush=True)
    sensitivity.reweight_arrays(ratio, logl, birth, run_start, nsamples=S, seed=1, device=0)
    rows, wall = [], []
    for _ in range(REPEATS):
        t = {}
        t0 = time.perf_counter()
        sensitivity.reweight_arrays(ratio, logl, birth, run_start, nsamples=S, seed=1, device=0, timing=t)
        wall.append(1e3 * (time.perf_counter() - t0))
        rows.append(t)
    print(f"  reweight (rvll_pointwise_replicates, {2 * len(alts)} units): setup {med(rows, 'setup_ms'):.2f} ms   weights "
          f"{med(rows, 'weights_ms'):.2f} ms   reduce {med(rows, 'reduce_ms'):.2f} ms   call {med(rows, 'total_ms'):.1f} ms   Python "
          f"call {float(np.median(wall)):.1f} ms", flush=True)


def main(R, gpu_only):
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    alts, labels = alternatives()
    runs, names, pri = [], [], []
    for k in range(MAX_PLANETS + 1):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            t0 = time.perf_counter()
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw)
            print(f"k = {k}: the {R} runs took {time.perf_counter() - t0:.0f} s", flush=True)
            runs.append(got)
            names.append(list(m.parnames))
            pri.append(dict(priordict))
        samples, logl, birth, run_start = pointwise._samples(got)
        print(f"k = {k}: R = {R} runs, {logl.size} merged rows, {len(names[k])} parameters, A = {len(alts)} alternatives, S = {S} "
              f"replicates with the run bootstrap; medians of {REPEATS} calls (min .. max)", flush=True)
        if k > 0:
            probe(k, samples, logl, birth, run_start, names[k], pri[k], alts, gpu_only)
    t0 = time.perf_counter()
    sens = sensitivity.sensitivity_per_model(runs, names, pri, alts, seed=1, nsamples=S, device=0)
    print(f"prior_sensitivity of the three models: {time.perf_counter() - t0:.1f} s", flush=True)
    pky = sensitivity.model_probabilities(sens)
    for k in range(1, MAX_PLANETS + 1):
        s = sens[k]
        print(f"k = {k}: ln Z = {s['logz_base']:.3f} +/- {s['logz_base_err']:.3f} under the base prior")
        for a in (0, 15, 31, 32, 47, 63):
            print(f"    {labels[a]}: dlnZ {s['dlogz'][a]:+.3f} +/- {s['dlogz_err'][a]:.3f} ({s['dlogz_min'][a]:+.3f} .. "
                  f"{s['dlogz_max'][a]:+.3f})   efficiency {s['efficiency'][a]:.3f}   outside {int(s['outside'][a])}")
    base = fip._softmax(np.array([s["logz_base"] for s in sens]))
    print("p(k | y), k = 0 .. 2, under the base prior: " + "  ".join(f"{p:.3e}" for p in base))
    with np.errstate(divide="ignore"):
        moved = np.argsort(-np.abs(np.log(pky["pky"][1]) - np.log(base[1])))[:5]
    for a in moved:
        print(f"    {labels[a]}: " + "  ".join(f"{pky['pky'][k, a]:.3e} +/- {pky['pky_err'][k, a]:.1e}" for k in range(MAX_PLANETS + 1)))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    main(int(args[0]) if args else 128, "--gpu-only" in sys.argv[1:])
