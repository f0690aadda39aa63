"""Parity of evidence_amd/nested.py with an earlier copy of itself: every driver configuration through both modules with the
same call-recording callbacks; every NestedResult field must have the same dtype, shape and bits (NaN included), `timing` the
same keys and `turns`, and the callbacks the same sequence of calls by name and batch shape.

    git show <commit>:evidence_amd/nested.py > /some/untracked/place/nested_parent.py
    python scripts/nested_parity.py /some/untracked/place/nested_parent.py            # the host matrix (toy models, fake live sets)
    python scripts/nested_parity.py /some/untracked/place/nested_parent.py --gpu      # the same forms on a one-planet GpuRVModel
    python scripts/nested_parity.py /some/untracked/place/nested_parent.py --time     # likelihood calls / s, both modules alternately

One line per configuration; exits non-zero at the first difference (--time: when the new module's median lies below the
earlier one's by more than that one's own max - min)."""
import argparse
import dataclasses
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from evidence_amd import nested as new  # noqa: E402


def load(path):
    """The file at path as a module of the package (its relative imports resolve inside evidence_amd)."""
    spec = importlib.util.spec_from_file_location("evidence_amd._nested_earlier", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def shapes(args):
    return tuple(np.shape(a) for a in args if isinstance(a, np.ndarray) or (isinstance(a, (list, tuple)) and len(a)))


class Log:
    """Wraps callables and live sets so that every call leaves (name, shapes of its array / sequence arguments)."""

    def __init__(self):
        self.calls = []

    def fn(self, name, f):
        if f is None:
            return None

        def call(*a, **k):
            self.calls.append((name, shapes(a), tuple(sorted(k))))
            return f(*a, **k)
        return call

    def live(self, obj):
        log = self

        class Proxy:
            def __getattr__(self, name):                 # (hasattr on the proxy is hasattr on the live set)
                attr = getattr(obj, name)
                return log.fn(name, attr) if callable(attr) else attr
        return Proxy()


def bits(x):
    if x is None or isinstance(x, (bool, int)):
        return (type(x).__name__, x)
    a = np.asarray(x)
    return (a.dtype.str, a.shape, a.tobytes())


def differences(a, b, la, lb):
    """What differs between two runs (NestedResult or list of them) and their call logs; empty when nothing does."""
    if isinstance(a, list):
        if len(a) != len(b):
            return ["number of results"]
        return [f"[{i}] {d}" for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, [], [])] + differences(None, None, la, lb)
    out = []
    if a is not None:
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            if f.name == "timing":
                if (x is None) != (y is None) or (x is not None and (set(x) != set(y) or x["turns"] != y["turns"])):
                    out.append("timing keys / turns")
            elif bits(x) != bits(y):
                out.append(f.name)
    if len(la) != len(lb):
        out.append(f"number of callback calls ({len(la)} / {len(lb)})")
    else:
        out += [f"callback call {i}: {x} / {y}" for i, (x, y) in enumerate(zip(la, lb)) if x != y][:1]
    return out


ONLY = None           # --only: run the configurations whose line holds this text


def both(old, name, run):
    """run(module, log) through both modules; prints the configuration's line, exits at a difference.  A configuration both
    modules refuse with the same error counts as equal (and says so)."""
    if ONLY and ONLY not in name:
        return
    got = []
    for mod in (old, new):
        log = Log()
        try:
            got.append((run(mod, log), log.calls))
        except Exception as exc:                         # noqa: BLE001
            got.append((f"{type(exc).__name__}: {exc}", log.calls))
    (a, la), (b, lb) = got
    if isinstance(a, str) or isinstance(b, str):
        diff = [] if a == b and la == lb else [f"errors: {a!r} / {b!r}"]
        what = f"both raise {a}"
    else:
        diff = differences(a, b, la, lb)
        first = a[0] if isinstance(a, list) else a
        what = f"niter {first.niter} ncall {first.ncall} logz {first.logz:.6f} calls {len(la)}"
    print(f"{name:78s} {'equal' if not diff else 'DIFFERENT: ' + '; '.join(diff)}   ({what})", flush=True)
    if diff:
        sys.exit(1)


# ---- the host matrix ---------------------------------------------------------------------------------------------------------
def host_matrix(old):
    import test_clustering_host as tc
    import test_nested_host as tn
    import test_nested_resident_clustering_host as trc
    import test_nested_resident_ensemble_host as tre
    from evidence_amd import adapt

    class AdaptiveRuns(trc._Runs):
        """The fake resident ensemble with per-run step counts and the walkers' distances (any deterministic numbers do: the
        drivers only count and compare them)."""
        _live_runs_step_steps = True

        def _distances(self, runs, kdead, ranks):
            before = [self.runs[int(r)].u.copy() for r in runs]
            return before, [np.argsort(self.runs[int(r)].logl, kind="stable") for r in runs]

        def _measure(self, runs, kdead, ranks, before, orders):
            move = np.stack([np.linalg.norm(self.runs[int(r)].u[o[:kdead]] - b[o[kdead:]][np.asarray(ranks[j])], axis=1)
                             for j, (r, b, o) in enumerate(zip(runs, before, orders))])
            pair = np.stack([np.full(kdead, np.std(b[o[kdead:]]) * (1.0 + 0.1 * j)) for j, (b, o) in enumerate(zip(before, orders))])
            return move, pair

        def live_runs_step(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=(), return_distances=False):
            per_run = np.broadcast_to(np.asarray(nsteps), (len(runs),))
            before, orders = self._distances(runs, kdead, ranks)
            run_list = self._take(runs, kdead, lstar)
            self.steps.append((run_list, None))
            got = [self.runs[r].step(kdead, ranks[j], lstar[j], wrapped, int(per_run[j]), seeds[j]) for j, r in enumerate(run_list)]
            out = (np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64))
            return out + self._measure(runs, kdead, ranks, before, orders) if return_distances else out

        def live_runs_step_clustered(self, runs, kdead, ranks, lstar, wrapped=None, nsteps=10, max_rounds=200, seeds=(), nboot=30,
                                     boot_seeds=(), return_distances=False):
            per_run = np.broadcast_to(np.asarray(nsteps), (len(runs),))
            before, orders = self._distances(runs, kdead, ranks)
            run_list = self._take(runs, kdead, lstar)
            self.steps.append((run_list, [int(b) for b in boot_seeds]))
            got = [self.runs[r].step(kdead, ranks[j], lstar[j], wrapped, int(per_run[j]), seeds[j], nboot, boot_seeds[j])
                   for j, r in enumerate(run_list)]
            out = (np.stack([g[0] for g in got]), np.array([g[1] for g in got], dtype=np.int64),
                   np.array([g[2] for g in got], dtype=np.int32))
            return out + self._measure(runs, kdead, ranks, before, orders) if return_distances else out

    def walker_runs_of(prior, loglike):
        wr = tc._WalkerRuns(prior, loglike)

        def call(cube, theta, logl, run_start, lstar, chol, wrapped, nsteps, max_rounds, seeds):
            per_group = np.broadcast_to(np.asarray(nsteps), (len(seeds),))          # adaptive runs pass one count per group
            if np.all(per_group == per_group[0]):
                return wr(cube, theta, logl, run_start, lstar, chol, wrapped, int(per_group[0]), max_rounds, seeds)
            parts = [wr(cube[run_start[g]:run_start[g + 1]], theta[run_start[g]:run_start[g + 1]], logl[run_start[g]:run_start[g + 1]],
                        np.array([0, run_start[g + 1] - run_start[g]]), lstar[g:g + 1], chol[g:g + 1], wrapped, int(per_group[g]),
                        max_rounds, seeds[g:g + 1]) for g in range(len(seeds))]
            return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
        return call

    models = [("gauss2", tc.gauss_prior, tc.gauss_loglike, 2, None),
              ("gauss3w", tc.gauss_prior, tc.gauss_loglike, 3, np.array([False, True, False])),
              ("bimodal3", tc.identity_prior, tc.mixture_loglike, 3, None)]
    for mname, prior, loglike, ndim, wrapped in models:
        bimodal = mname == "bimodal3"
        for kbatch in (1, 15, 59):
            base = dict(nlive=60, kbatch=kbatch, nsteps=4, dlogz=0.1, wrapped=wrapped, max_calls=1500 if kbatch == 1 else 5000)
            fused = lambda c: (prior(c), loglike(prior(c)))                                          # noqa: E731
            single = lambda *a: tc._walk(*a, prior=prior, loglike=loglike)                           # noqa: E731

            def one(name, seeds=(5,), ensemble=False, use=(), **kw):
                """A configuration: run_nested_slice for the one seed, or run_nested_ensemble(seeds)."""
                def run(mod, log):
                    k = dict(base, **kw)
                    for key in use:
                        k[key] = {"walker": lambda: log.fn("walker", single),
                                  "walker_runs": lambda: log.fn("walker_runs", walker_runs_of(prior, loglike)),
                                  "prior_loglike": lambda: log.fn("prior_loglike", fused),
                                  "clusterer": lambda: log.fn("clusterer", new._default_clusterer(None)),
                                  "distances": lambda: log.fn("distances", adapt.walk_distances_runs)}[key]()
                    if "live" in k:
                        k["live"] = log.live(k["live"]())
                        p = ll = None
                    else:
                        p, ll = log.fn("prior", prior), log.fn("loglike", loglike)
                    if ensemble:
                        return mod.run_nested_ensemble(p, ll, ndim, list(seeds), **k)
                    return mod.run_nested_slice(p, ll, ndim, seed=seeds[0], **k)
                both(old, f"{mname} kbatch={kbatch:2d} {name}" + (f" seeds={len(seeds)}" if ensemble else ""), run)

            if not bimodal:
                one("host chord walk")
                one("host stepout walk", proposal="stepout", step_width=0.8)
                one("host chord walk, prior_loglike=", use=["prior_loglike"])
                one("host stepout walk, prior_loglike=", use=["prior_loglike"], proposal="stepout")
                one("walker=", use=["walker"])
                one("walker_runs=", use=["walker_runs"])
                one("adaptive, host walk", use=["distances"], adaptive_nsteps="move-distance", max_nsteps=9)
                one("adaptive, walker=", use=["walker", "distances"], adaptive_nsteps="move-distance", max_nsteps=9)
                one("adaptive, walker_runs=", use=["walker_runs", "distances"], adaptive_nsteps="move-distance", max_nsteps=9)
                one("precision_criterion, host walk", precision_criterion=0.05)
                one("precision_criterion, walker_runs=", use=["walker_runs"], precision_criterion=0.05)
                one("max_iter cut, host walk", max_iter=5 * kbatch)
                one("max_iter cut, walker=", use=["walker"], max_iter=5 * kbatch)
            one("clustering, host walk", use=["clusterer"], clustering=True, nboot=8)
            one("clustering, host stepout walk", use=["clusterer"], clustering=True, nboot=8, proposal="stepout")
            one("clustering, walker_runs=", use=["clusterer", "walker_runs"], clustering=True, nboot=8)
            one("clustering + adaptive, host walk", use=["clusterer", "distances"], clustering=True, nboot=8,
                adaptive_nsteps="move-distance", max_nsteps=9)
            one("clustering + adaptive, walker_runs=", use=["clusterer", "distances", "walker_runs"], clustering=True, nboot=8,
                adaptive_nsteps="move-distance", max_nsteps=9)
            one("region", use=["clusterer"], proposal="region", nboot=8)
            one("region, prior_loglike=", use=["clusterer", "prior_loglike"], proposal="region", nboot=8)
            one("region, walker_runs=", use=["clusterer", "walker_runs"], proposal="region", nboot=8, region_max_candidates=64)
            one("region, every point from the fallback walk", use=["clusterer"], proposal="region", nboot=8, region_max_candidates=0)
            one("region, fallback through walker_runs=", use=["clusterer", "walker_runs"], proposal="region", nboot=8,
                region_max_candidates=0)
            one("region, precision_criterion", use=["clusterer"], proposal="region", nboot=8, precision_criterion=0.05)
            for n in (1, 3, 7):
                seeds = list(range(11, 11 + n))
                one("ensemble walker_runs=", seeds, True, use=["walker_runs"])
                one("ensemble clustering", seeds, True, use=["clusterer", "walker_runs"], clustering=True, nboot=8)
                one("ensemble adaptive", seeds, True, use=["distances", "walker_runs"], adaptive_nsteps="move-distance", max_nsteps=9)
                one("ensemble clustering + adaptive", seeds, True, use=["clusterer", "distances", "walker_runs"], clustering=True,
                    nboot=8, adaptive_nsteps="move-distance", max_nsteps=9)
                one("ensemble region", seeds, True, use=["clusterer"], proposal="region", nboot=8)
                one("ensemble region, walker_runs=", seeds, True, use=["clusterer", "walker_runs"], proposal="region", nboot=8,
                    region_max_candidates=64)
                one("ensemble region, fallback walk only", seeds, True, use=["clusterer"], proposal="region", nboot=8,
                    region_max_candidates=0)
                if n > 1:
                    # max_calls between the runs' needs: one leaves the lockstep early
                    one("ensemble, max_calls stops a run early", seeds, True, use=["walker_runs"], max_calls=1000, dlogz=1e-6)
                    one("ensemble region, max_calls stops a run early", seeds, True, use=["clusterer"], proposal="region", nboot=8,
                        max_calls=1000, dlogz=1e-6)
                one("ensemble max_iter cut", seeds, True, use=["walker_runs"], max_iter=5 * kbatch)
                one("ensemble precision_criterion", seeds, True, use=["walker_runs"], precision_criterion=0.05)
                fake = lambda: trc._Runs(trc._Model(prior, loglike))                                 # noqa: E731
                one("resident ensemble (fake live sets)", seeds, True, live=fake)
                one("resident ensemble, clustered", seeds, True, live=fake, clustering=True, nboot=8)
                one("resident ensemble, precision_criterion", seeds, True, live=fake, precision_criterion=0.05)
                adaptive = lambda: AdaptiveRuns(trc._Model(prior, loglike))                          # noqa: E731
                one("resident ensemble, adaptive", seeds, True, live=adaptive, adaptive_nsteps="move-distance", max_nsteps=9)
                one("resident ensemble, clustered + adaptive", seeds, True, live=adaptive, clustering=True, nboot=8,
                    adaptive_nsteps="move-distance", max_nsteps=9)
            one("resident one run, clustered", live=fake, clustering=True, nboot=8)
            one("resident one run, adaptive", live=adaptive, adaptive_nsteps="move-distance", max_nsteps=9)
            if mname == "gauss2" or mname == "gauss3w":
                # the one-run fake live sets of the host tests walk the Gaussian in its box
                host_live = lambda: tn._HostLive(prior, loglike, single)                             # noqa: E731
                sorting = lambda: tn._HostLiveSorting(prior, loglike, single)                        # noqa: E731
                for pc in (None, 0.05):
                    tag = "" if pc is None else ", precision_criterion"
                    one('resident one run, live_chol="host"' + tag, live=host_live, live_chol="host", precision_criterion=pc)
                    one('resident one run, live_chol="device"' + tag, live=host_live, precision_criterion=pc)
                    one("resident one run, device order" + tag, live=sorting, precision_criterion=pc)
                one("resident one run, device order, max_iter cut", live=sorting, max_iter=5 * kbatch)
                if ndim == 3 and wrapped is None:
                    one("resident one run, device order (ensemble tests' fake)", live=tre._OneRun)
    # the ellipsoid sampler takes the shared result builder
    for ndim in (2, 3):
        def run(mod, log):
            return mod.run_nested(log.fn("prior", tc.gauss_prior), log.fn("loglike", tc.gauss_loglike), ndim, nlive=60, seed=2)
        both(old, f"run_nested ndim={ndim}", run)

        def run(mod, log):
            return mod.run_nested(log.fn("prior", tc.gauss_prior), log.fn("loglike", tc.gauss_loglike), ndim, nlive=60, seed=2,
                                  max_calls=700, batch=64)
        both(old, f"run_nested ndim={ndim}, max_calls ends it", run)


# ---- the GPU matrix ------------------------------------------------------------------------------------------------------------
def gpu_model(cfg):
    from evidence_amd import GpuRVModel
    from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
    from evidence_amd.synthetic import make_workload
    w = make_workload(cfg)
    m = GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict())
    prior, loglike = make_ultranest_callbacks(m, vectorized=True)
    return m, prior, loglike, wrapped_params(m.parnames)


def gpu_matrix(old):
    m, prior, loglike, wrapped = gpu_model(2)                   # one planet
    with m:
        def one(name, seeds, ensemble=False, use=(), max_calls=40_000, **kw):
            def run(mod, log):
                k = dict(nlive=400, kbatch=100, wrapped=wrapped, max_calls=max_calls, **kw)
                for key in use:
                    k[key] = log.fn(key, {"walker": m.slice_walk, "walker_runs": m.slice_walk_runs, "prior_loglike": m.prior_loglike_batch,
                                          "clusterer": m.cluster_runs, "distances": m.walk_distances_runs,
                                          "region_runs": m.region_draw_runs}[key])
                if "live" in k:
                    k["live"] = log.live(m)
                p, ll = log.fn("prior", prior), log.fn("loglike", loglike)
                if ensemble:
                    return mod.run_nested_ensemble(p, ll, m.ndim, list(seeds), **k)
                return mod.run_nested_slice(p, ll, m.ndim, seed=seeds[0], **k)
            both(old, f"gpu {name}" + (f" seeds={list(seeds)}" if ensemble else f" seed={seeds[0]}"), run)

        adaptive = dict(adaptive_nsteps="move-distance", max_nsteps=40)
        for s in (1, 2, 3):
            one("host chord walk, prior_loglike=", [s], use=["prior_loglike"], max_calls=8000)
            one("host stepout walk, prior_loglike=", [s], use=["prior_loglike"], max_calls=8000, proposal="stepout")
            one("walker=", [s], use=["walker", "prior_loglike"])
            one("walker=, stepout", [s], use=["walker"], proposal="stepout")
            one("walker=, precision_criterion", [s], use=["walker"], precision_criterion=0.5)
            one("walker_runs=", [s], use=["walker_runs"])
            one("clustering, walker_runs=", [s], use=["walker_runs", "clusterer"], clustering=True)
            one("adaptive, walker=", [s], use=["walker", "distances"], **adaptive)
            one("clustering + adaptive, walker_runs=", [s], use=["walker_runs", "clusterer", "distances"], clustering=True, **adaptive)
            one("region", [s], use=["clusterer", "region_runs", "walker_runs"], proposal="region")
            one("region, fallback walk only", [s], use=["clusterer", "region_runs", "walker_runs"], proposal="region",
                region_max_candidates=0)
            one('live=, live_chol="host"', [s], live=True, live_chol="host")
            one("live= (device order)", [s], live=True)
            one("live=, stepout, precision_criterion", [s], live=True, proposal="stepout", precision_criterion=0.5)
            one("live=, clustering", [s], live=True, clustering=True)
            one("live=, adaptive", [s], live=True, **adaptive)
        for seeds in ([1], [1, 2, 3]):
            one("ensemble walker_runs=", seeds, True, use=["walker_runs"], max_calls=40_000)
            one("ensemble clustering", seeds, True, use=["walker_runs", "clusterer"], clustering=True)
            one("ensemble adaptive", seeds, True, use=["walker_runs", "distances"], **adaptive)
            one("ensemble clustering + adaptive", seeds, True, use=["walker_runs", "clusterer", "distances"], clustering=True, **adaptive)
            one("ensemble region", seeds, True, use=["clusterer", "region_runs", "walker_runs"], proposal="region")
            one("ensemble live=", seeds, True, live=True)
            one("ensemble live=, clustering", seeds, True, live=True, clustering=True)
            one("ensemble live=, adaptive", seeds, True, live=True, **adaptive)
            one("ensemble live=, clustering + adaptive", seeds, True, live=True, clustering=True, **adaptive)


# ---- speed -------------------------------------------------------------------------------------------------------------------
def timing(old):
    """bench.py's end-to-end configuration (resident and walker=) and an 8-seed walker_runs ensemble at 2048 live points:
    a warm-up, then the earlier module and this one alternately, three times each."""
    m, prior, loglike, wrapped = gpu_model(3)
    ok = True
    with m:
        end = dict(nlive=32768, kbatch=16384, dlogz=1e-9, max_calls=60_000_000, wrapped=wrapped, seed=1)
        forms = [("end to end, resident (live=)", lambda mod: mod.run_nested_slice(None, None, m.ndim, live=m, **end)),
                 ("end to end, host-managed (walker=)",
                  lambda mod: mod.run_nested_slice(prior, loglike, m.ndim, prior_loglike=m.prior_loglike_batch, walker=m.slice_walk, **end)),
                 ("ensemble of 8 seeds, walker_runs=, 2048 live points",
                  lambda mod: mod.run_nested_ensemble(prior, loglike, m.ndim, list(range(1, 9)), nlive=2048, kbatch=512, dlogz=1e-9,
                                                      max_calls=1_500_000, wrapped=wrapped, walker_runs=m.slice_walk_runs))]
        for name, run in forms:
            def rate(mod):
                t0 = time.perf_counter()
                res = run(mod)
                el = time.perf_counter() - t0
                return sum(r.ncall for r in res) / el if isinstance(res, list) else res.ncall / el
            rate(new)                                           # warm-up
            rates = {"earlier": [], "new": []}
            for _ in range(3):
                rates["earlier"].append(rate(old))
                rates["new"].append(rate(new))
            for who, r in rates.items():
                print(f"{name:55s} {who:8s} calls/s: " + "  ".join(f"{v:.4e}" for v in r) + f"   median {np.median(r):.4e}", flush=True)
            spread = max(rates["earlier"]) - min(rates["earlier"])
            short = np.median(rates["earlier"]) - np.median(rates["new"])
            fine = short <= spread
            ok = ok and fine
            print(f"{name:55s} new median below the earlier one by {short:.3e}, allowed {spread:.3e} (its max - min): "
                  f"{'ok' if fine else 'SLOWER'}", flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("earlier", help="the earlier nested.py (git show <commit>:evidence_amd/nested.py > FILE), kept out of git")
    ap.add_argument("--gpu", action="store_true", help="the GPU matrix instead of the host one")
    ap.add_argument("--time", action="store_true", help="likelihood calls per second of both modules")
    ap.add_argument("--only", help="only the configurations whose name holds this text")
    args = ap.parse_args()
    ONLY = args.only
    earlier = load(args.earlier)
    (timing if args.time else gpu_matrix if args.gpu else host_matrix)(earlier)
    print("all equal")
