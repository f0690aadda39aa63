#!/usr/bin/env python3
"""Equal-weight draws and curve bands of merged runs: R = 128 resident clustered runs of the 51 Peg example
(examples/51peg/config_51peg.py, k = 1 and 2 planets, 400 live points, dlogz 0.5), S = 1000 replicates with the run bootstrap,
n = 256 draws a replicate, the curve of planet 1 at T = 512 times over one period.  Medians of REPEATS calls after a warm-up call:
    draws       draws.draw(device=0): rvll_draw_replicates — HIP-event time by phase (setup: the merge's; weights: the replicate
                kernels; scan: fixed point and the running sum; pick: the searches) and the whole C call
    bands       GpuRVModel.kep_rv_bands on the S x n drawn rows: HIP-event time of the curve kernel and of the sort, and the wall
                time of the call with its upload and downloads
    new route   predictive.curve_bands(device=0), wall
    parent      the route without this code, on the same card: merge.replicates(return_logwt=True, device=0) in blocks of
                PARENT_BLOCK replicates (the weights cross to the host), exp / cumsum / searchsorted, kep_rv_batch and np.sort on
                the host — timed on PARENT_REPS replicates and scaled to S (labelled as scaled); --full-parent runs all S
Run on the GPU box:  python3 scripts/predictive_probe.py [--full-parent] [R [output]]; the text goes to
profiles/predictive_probe.txt unless an output path is given."""
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from evidence_amd import GpuRVModel, draws, merge, predictive, run_nested_ensemble  # noqa: E402
from evidence_amd.callbacks import wrapped_params  # noqa: E402
from evidence_amd.config import read_config  # noqa: E402

S, NDRAWS, NTIMES = 1000, 256, 512
PARENT_REPS, PARENT_BLOCK = 100, 20
REPEATS = 3
LEVELS = predictive.QUANTILES


def med(rows, key):
    return float(np.median([r[key] for r in rows]))


def parent_route(results, model, times, nsamples, seed):
    """Bands of the planet's curve with what the parent commit has: the replicated weights come to the host block by block."""
    _, logl, birth, run_start = merge._stack(results)
    stacked = np.concatenate([np.asarray(r.samples, dtype=np.float64).reshape(len(r.logl), -1) for r in results])
    order = merge.merge_arrays(logl, birth, run_start, device=0)["order"]
    rng = np.random.default_rng(seed)
    q = np.empty((nsamples, len(LEVELS), times.shape[0]))
    for s0 in range(0, nsamples, PARENT_BLOCK):
        sb = min(PARENT_BLOCK, nsamples - s0)
        # replicates s0 .. s0 + sb of the call with `seed`: the seed of replicate s is seed + s SEED_MUL
        block_seed = int(merge.replicate_seeds(seed, s0 + 1)[s0])
        logwt = merge.replicates_arrays(logl, birth, run_start, sb, seed=block_seed, device=0, return_logwt=True)[2]
        for s in range(sb):
            with np.errstate(invalid="ignore"):
                c = np.cumsum(np.exp(logwt[s]))
            u = (rng.random() + np.arange(NDRAWS)) / NDRAWS * c[-1]
            rows = order[np.minimum(np.searchsorted(c, u, side="right"), c.shape[0] - 1)]
            curves = model.modelk_batch(stacked[rows], times, 1)
            srt = np.sort(curves, axis=0)
            for k, lv in enumerate(LEVELS):
                q[s0 + s, k] = srt[max(0, int(np.ceil(lv * NDRAWS)) - 1)]
    return q.mean(axis=0), q.std(axis=0)


def main(R, full_parent, out):
    def say(text=""):
        print(text, flush=True)
        out.write(text + "\n")
        out.flush()

    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (1, 2):
        probe(k, R, full_parent, cfg, say)


def probe(k, R, full_parent, cfg, say):
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        names = list(m.parnames)
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, R + 1)), live=m, clustering=True, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=60_000_000)
        n_rows = sum(len(g.logl) for g in got)
        period = float(np.median(np.concatenate([np.asarray(g.samples)[-50:, names.index("planet1_period")] for g in got])))
        times = 50000.0 + np.linspace(0.0, period, NTIMES)
        say(f"k = {k}: R = {R} runs, {n_rows} merged rows, S = {S} replicates (run bootstrap, random shrinkage), n = {NDRAWS} draws a "
            f"replicate, T = {NTIMES} times over one period of {period:.5f} d; medians of {REPEATS} calls after a warm-up")

        draws.draw(got, NDRAWS, S, seed=1, device=0)
        dt = []
        for _ in range(REPEATS):
            t = {}
            rows, logz, _ = draws.draw(got, NDRAWS, S, seed=1, device=0, timing=t)
            dt.append(t)
        say(f"  draws (rvll_draw_replicates):  kernels {med(dt, 'kernel_ms'):9.2f} ms ({min(r['kernel_ms'] for r in dt):.2f} .. "
            f"{max(r['kernel_ms'] for r in dt):.2f})   call {med(dt, 'total_ms'):9.1f} ms   in {dt[0]['blocks']} blocks of "
            f"replicates, {dt[0]['tiles']} tiles, {dt[0]['launches']} launches")
        say(f"      setup {med(dt, 'setup_ms'):8.2f} ms   weights {med(dt, 'weights_ms'):8.2f} ms   scan {med(dt, 'scan_ms'):8.2f} ms"
            f"   pick {med(dt, 'pick_ms'):8.2f} ms")
        say(f"      scan per (row, replicate) {1e9 * med(dt, 'scan_ms') / (n_rows * S):.2f} ps   pick per draw "
            f"{1e6 * med(dt, 'pick_ms') / (NDRAWS * S):.2f} ns   replicates with draws {int((rows[:, 0] >= 0).sum())} of {S}")

        theta = draws.samples(got, NDRAWS, S, seed=1, device=0)
        m.kep_rv_bands(theta, times, LEVELS, planet=1)
        bt = []
        for _ in range(REPEATS):
            t = {}
            t0 = time.perf_counter()
            m.kep_rv_bands(theta, times, LEVELS, planet=1, timing=t)
            t["wall_ms"] = 1e3 * (time.perf_counter() - t0)
            bt.append(t)
        nvals = S * NDRAWS * NTIMES
        say(f"  bands (rvll_kep_rv_bands):     curves {med(bt, 'curves_ms'):9.2f} ms   sort {med(bt, 'sort_ms'):9.2f} ms   call "
            f"{med(bt, 'wall_ms'):9.1f} ms   for {nvals:.3g} curve values: curves {1e6 * med(bt, 'curves_ms') / nvals:.3f} ns, sort "
            f"{1e6 * med(bt, 'sort_ms') / nvals:.3f} ns a value")

        predictive.curve_bands(got, m, times, planet=1, ndraws=NDRAWS, nsamples=S, seed=1, device=0)
        walls = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            new = predictive.curve_bands(got, m, times, planet=1, ndraws=NDRAWS, nsamples=S, seed=1, device=0)
            walls.append(time.perf_counter() - t0)
        new_s = float(np.median(walls))
        say(f"  new route (predictive.curve_bands, device=0):  wall {new_s:8.3f} s   median-curve amplitude "
            f"{0.5 * (new['band'][1].max() - new['band'][1].min()):.3f} m/s, largest band_err {new['band_err'].max():.3f} m/s")

        reps = S if full_parent else PARENT_REPS
        t0 = time.perf_counter()
        band, err = parent_route(got, m, times, reps, 1)
        parent_s = (time.perf_counter() - t0) * S / reps
        label = "measured on all replicates" if full_parent else f"scaled from {reps} replicates (x {S // reps})"
        say(f"  parent route (weights to the host, {8e-9 * n_rows * S:.1f} GB at S = {S}; searchsorted, kep_rv_batch, np.sort):  wall "
            f"{parent_s:8.1f} s, {label}   median-curve amplitude {0.5 * (band[1].max() - band[1].min()):.3f} m/s, largest "
            f"band_err {err.max():.3f} m/s")
        say(f"  new route / parent route: {new_s / parent_s:.4f}   (the new route is {'faster' if new_s < parent_s else 'NOT faster'})")
        say()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = Path(args[1]) if len(args) > 1 else Path(__file__).resolve().parents[1] / "profiles" / "predictive_probe.txt"
    with open(path, "w") as fh:
        main(int(args[0]) if args else 128, "--full-parent" in sys.argv[1:], fh)
