#!/usr/bin/env python3
"""The clustering of live points (rvll_cluster_runs) measured two ways.  Run on the GPU box:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 scripts/cluster_probe.py --kernels
    python3 scripts/cluster_probe.py --parse OUT        kernel times per shape from that trace
    python3 scripts/cluster_probe.py [R]                 51 Peg, k = 1 and 2, R runs (default 32) with and without clustering

--kernels: R x n = 1 x 400, 128 x 400 and 1 x 8192 uniform rows at D = 7 and 19 with B = 30, 20 calls each after a warm-up
(the wall time of one call, upload to download, is printed).  --parse: the device time of the three kernels of a call, median
over the calls of a shape (shapes told apart by the row kernels' grid and the dimension bound of their instantiation).
The 51 Peg part: run_nested_ensemble(walker_runs=model.slice_walk_runs) with clustering off and on (clusterer =
model.cluster_runs): ln Z median and standard deviation over the runs, likelihood calls, wall time, the cluster counts seen."""
import csv
import glob
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

SHAPES = [(1, 400), (128, 400), (1, 8192)]


def kernels():
    from evidence_amd import GpuRVModel
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    for D in (7, 19):
        names = [f"i{k}" for k in range(D)]
        table = EpochTable.from_arrays(names, np.arange(1.0, D + 1.0), np.zeros(D), np.ones(D), np.arange(D))
        pri = {f"{n}_offset": P.Uniform(-10, 10) for n in names}
        with GpuRVModel({}, table, list(pri), priordict=pri) as m:
            rng = np.random.default_rng(D)
            for R, n in SHAPES:
                cube = rng.random((R * n, D))
                run_start = np.arange(R + 1, dtype=np.int64) * n
                scale = np.full((R, D), np.sqrt(12.0))
                m.cluster_runs(cube, run_start, scale, None, 30, range(R))
                t = []
                for k in range(20):
                    t0 = time.perf_counter()
                    _, ncl, _ = m.cluster_runs(cube, run_start, scale, None, 30, range(k, k + R))
                    t.append(time.perf_counter() - t0)
                print(f"D {D:>2}  R x n {R:>3} x {n:<5} wall per call {1e3 * np.median(t):8.3f} ms (median of 20)  "
                      f"clusters {int(ncl.min())} .. {int(ncl.max())}", flush=True)


def parse(out):
    rows = []
    for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "cluster_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # a call = nn, link, label (nn and link only when some run has rows): group them by the call's label launch
    calls, cur = [], []
    for r in rows:
        cur.append(r)
        if "cluster_label_kernel" in r["Kernel_Name"]:
            calls.append(cur)
            cur = []
    shapes = {}
    for c in calls:
        nn = [r for r in c if "cluster_nn_kernel" in r["Kernel_Name"]][0]
        blocks = int(nn["Grid_Size_X"]) // int(nn["Workgroup_Size_X"]) if "Grid_Size_X" in nn else int(nn["Grid_Size"]) // int(nn["Workgroup_Size"])
        dm = nn["Kernel_Name"].split("<")[1].split(">")[0]
        ns = {k: int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in c
              for k in ("nn", "link", "label") if f"cluster_{k}_kernel" in r["Kernel_Name"]}
        shapes.setdefault((dm, blocks), []).append((ns["nn"], ns["link"], ns["label"], int(c[-1]["End_Timestamp"]) - int(c[0]["Start_Timestamp"])))
    for (dm, blocks), v in sorted(shapes.items()):
        v = np.array(v[1:]) / 1e3                      # the warm-up call out
        med = np.median(v, axis=0)
        print(f"D bound {dm:>2}, {blocks:>4} row workgroups: nn {med[0]:8.1f} us  link {med[1]:8.1f} us  label {med[2]:7.1f} us  "
              f"first launch to last end {med[3]:8.1f} us  ({len(v)} calls)")


def peg(R):
    from evidence_amd import GpuRVModel, run_nested_ensemble
    from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    for k in (1, 2):
        rundict, datadict, priordict, fixed = read_config(cfg, nplanets=k)
        with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
            prior, loglike = make_ultranest_callbacks(m, vectorized=True)
            kw = dict(nlive=400, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=60_000_000,
                      walker_runs=m.slice_walk_runs)
            run_nested_ensemble(prior, loglike, m.ndim, [999, 998], clusterer=m.cluster_runs, clustering=True, **kw)   # warm-up
            print(f"51 Peg, k = {k}, ndim {m.ndim}, nlive 400, dlogz 0.5, R = {R} runs", flush=True)
            for on in (False, True):
                t0 = time.perf_counter()
                out = run_nested_ensemble(prior, loglike, m.ndim, list(range(1, R + 1)), clustering=on,
                                          clusterer=m.cluster_runs if on else None, **kw)
                wall = time.perf_counter() - t0
                lz = np.array([r.logz for r in out])
                line = (f"  clustering {'on ' if on else 'off'}: ln Z median {np.median(lz):9.3f} std {lz.std():7.3f} "
                        f"(min {lz.min():9.3f} max {lz.max():9.3f}); calls {sum(r.ncall for r in out):>12,}; "
                        f"iterations {min(r.niter for r in out)} .. {max(r.niter for r in out)}; wall {wall:6.2f} s")
                if on:
                    ncl = np.concatenate([r.nclusters for r in out])
                    counts = np.bincount(ncl)
                    line += "; clusters per iteration: " + ", ".join(f"{c}: {n}" for c, n in enumerate(counts) if n)
                print(line, flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--kernels"]:
        kernels()
    elif sys.argv[1:2] == ["--parse"]:
        parse(sys.argv[2])
    else:
        peg(int(sys.argv[1]) if len(sys.argv) > 1 else 32)
