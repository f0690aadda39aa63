#!/usr/bin/env python3
"""Marginal histograms of merged runs with both error bars: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, kbatch 100, dlogz 0.5), every parameter as a 1-D panel of
200 bins and every pair as a 40 x 40 panel, over S = 1000 replicates with the run bootstrap (k = 2: planets ordered by period
first).  Edges as marginals.marginals chooses them.  Per k, medians of REPEATS calls after a warm-up call:
    histograms      marginals.marginals_arrays(device=0): rvll_marginal_replicates — HIP-event time in all and of its three parts
                    (setup: merge setup, bin table, counts; weights: the replicate kernels; reduce: fixed point, the histogram
                    kernel, the statistics), the whole C call; then the reduce time with the wave-level pre-reduction switched
                    on (RVLL_MARGINAL_WAVE_REDUCE=1 in the environment; the bits must not change)
    yardstick       posterior.summarize_arrays(device=0): rvll_posterior_replicates' reduce_ms on the same rows and columns — the
                    three-pass summary with its gather, code that the histogram work does not touch — and the ratio of the two
                    reduce times per (row, replicate, panel) and per (row, replicate, column)
    numpy           the definition (device=None) timed on NUMPY_REPS replicates and scaled to S (labelled as scaled)
then the largest error of a 1-D bin near the period peak with the run bootstrap and from simulated shrinkage alone.
Run on the GPU box:  python3 scripts/marginals_probe.py [--gpu-only] [R]; the text goes to profiles/marginals_probe.txt."""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, marginals, posterior, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S = 1000
NUMPY_REPS = 2
REPEATS = 3
BINS_1D, BINS_2D = 200, 40


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def panels_for(cols, names, logl, birth, run_start):
    rng = posterior.summarize_arrays(cols, logl, birth, run_start, marginals.RANGE_QUANTILES, 1, 0, "expected", False, 0)
    rng = rng["quantiles"][0]
    ncols = cols.shape[1]
    axes = [(c, marginals._edges(rng[0, c], rng[1, c], BINS_1D, "period" in names[c])) for c in range(ncols)]
    axes += [(c, marginals._edges(rng[0, c], rng[1, c], BINS_2D, "period" in names[c])) for c in range(ncols)]
    return axes, list(range(ncols)) + [(ncols + a, ncols + b) for a in range(ncols) for b in range(a + 1, ncols)]


def main(R, gpu_only, out):
    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            names = list(m.parnames)
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
            got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, **kw)
        _, cols, logl, birth, run_start = posterior._values(got, None, None, k > 1, names)
        n, ncols = cols.shape
        axes, panels = panels_for(cols, names, logl, birth, run_start)
        args = (cols, logl, birth, run_start, axes, panels)
        marginals.marginals_arrays(*args, nsamples=S, seed=1, device=0)                              # warm-up at the timed shape
        posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=S, seed=1, device=0)
        mt, pt = [], []
        for _ in range(REPEATS):                                                 # the two entries alternate
            t = {}
            boot = marginals.marginals_arrays(*args, nsamples=S, seed=1, device=0, timing=t)
            mt.append(t)
            t = {}
            posterior.summarize_arrays(cols, logl, birth, run_start, nsamples=S, seed=1, device=0, timing=t)
            pt.append(t)
        os.environ["RVLL_MARGINAL_WAVE_REDUCE"] = "1"
        plain = []
        for _ in range(REPEATS):
            t = {}
            flat = marginals.marginals_arrays(*args, nsamples=S, seed=1, device=0, timing=t)
            plain.append(t)
        del os.environ["RVLL_MARGINAL_WAVE_REDUCE"]
        same = all(np.array_equal(boot[key], flat[key]) for key in boot)
        npan, nbins = len(panels), int(boot["panel_start"][-1])
        say(f"k = {k}: R = {R} runs, {n} merged rows, {ncols} columns, {npan} panels ({ncols} of {BINS_1D} bins, {npan - ncols} of "
            f"{BINS_2D} x {BINS_2D}), {nbins} bins, S = {S} replicates; medians of {REPEATS} calls (min .. max of the kernel time)")
        say(f"  histograms (rvll_marginal_replicates):   kernels {med(mt, 'kernel_ms'):9.2f} ms "
            f"({min(r['kernel_ms'] for r in mt):.2f} .. {max(r['kernel_ms'] for r in mt):.2f})   call {med(mt, 'total_ms'):9.1f} ms")
        say(f"      setup {med(mt, 'setup_ms'):8.2f} ms   weights {med(mt, 'weights_ms'):8.2f} ms   reduce "
            f"{med(mt, 'reduce_ms'):8.2f} ms   in {mt[0]['blocks']} blocks of replicates, {mt[0]['groups']} panel groups, "
            f"{mt[0]['launches']} launches")
        say(f"      with the wave-level pre-reduction:    reduce {med(plain, 'reduce_ms'):8.2f} ms   same bits: {same}")
        say(f"  yardstick (rvll_posterior_replicates):   kernels {med(pt, 'kernel_ms'):9.2f} ms   reduce "
            f"{med(pt, 'reduce_ms'):8.2f} ms for {ncols} columns, {pt[0]['blocks']} blocks")
        per_panel = med(mt, "reduce_ms") / npan
        per_col = med(pt, "reduce_ms") / ncols
        say(f"      reduce per (row, replicate, panel) {1e9 * per_panel / (n * S):.2f} ps   per (row, replicate, column) "
            f"{1e9 * per_col / (n * S):.2f} ps   ratio histogram / summary {per_panel / per_col:.3f}")
        if not gpu_only:
            t0 = time.perf_counter()
            ref = marginals.marginals_arrays(*args, nsamples=NUMPY_REPS, seed=1, return_replicates=True)
            numpy_s = (time.perf_counter() - t0) * S / NUMPY_REPS
            dev = marginals.marginals_arrays(*args, nsamples=NUMPY_REPS, seed=1, device=0, return_replicates=True)
            err = float(np.max(np.abs(dev["mass"] - ref["mass"])))
            say(f"  numpy definition: {numpy_s:.0f} s scaled from {NUMPY_REPS} replicates (x {S // NUMPY_REPS}); device against it "
                f"there: counts equal {np.array_equal(dev['counts'], ref['counts'])}, max |mass err| {err:.1e}")
        shrink = marginals.marginals_arrays(*args, nsamples=S, seed=1, device=0, bootstrap=False)
        for c in [i for i, name in enumerate(names) if "period" in name]:
            sl = slice(int(boot["panel_start"][c]), int(boot["panel_start"][c + 1]))
            top = int(np.argmax(boot["mean"][sl]))
            near = slice(sl.start + max(top - 5, 0), sl.start + min(top + 6, BINS_1D))
            j = int(np.argmax(boot["std"][near]))
            e = axes[c][1]
            say(f"  {names[c]}: peak bin [{e[top]:.7f}, {e[top + 1]:.7f}] mass {boot['mean'][sl][top]:.4f}; largest error within 5 "
                f"bins of it: bootstrap {boot['std'][near][j]:.2e} (mass {boot['mean'][near][j]:.4f}, min "
                f"{boot['min'][near][j]:.4f}, max {boot['max'][near][j]:.4f}), shrinkage only {shrink['std'][near].max():.2e}")
        say()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--gpu-only"]
    path = Path(__file__).resolve().parents[1] / "profiles" / "marginals_probe.txt"
    with open(path, "w") as fh:
        main(int(args[0]) if args else 128, "--gpu-only" in sys.argv[1:], fh)
