"""Parity of the device walk's host driver (evidence_amd/csrc/rvll_walk_host.hip, rvll_walk_plan.h) with an earlier build of the
library: a fixed matrix of walks through both libraries — cfg 1, 3 and 5; 40 to 40000 walkers; the slim table range at 30 and at 1
(walkers deferred to the full-solver finish); the chord walk under every switch variant of the rounds and single-kernel forms, the
stepout walk, run mode with a uniform and a mixed step table — comparing a digest of the end points' cube, theta and log-L, the
likelihood calls, rvll_slice_walk_evaluated, rvll_slice_walk_rounds and the `[rounds]` geometry line of RVLL_WALK_GEOM_DUMP.

    git worktree add /some/untracked/place <commit> && make -C /some/untracked/place/evidence_amd/csrc
    python scripts/walk_host_parity.py /some/untracked/place/evidence_amd/librvll.so            # the matrix
    python scripts/walk_host_parity.py /some/untracked/place/evidence_amd/librvll.so --time     # calls / s inside the walk
    python scripts/walk_host_parity.py EARLIER.so EARLIER.so --keep-going       # a build against itself: what is reproducible at all

Each library is loaded (RVLL_LIBRARY) in a fresh child process under a time limit.  One line per walk; exits with status 1 at the
first difference (--keep-going: after the last walk, having listed every difference), with status 3 at a child that fails or does
not end (--time: status 1 when this build's median lies below the earlier one's by more than that one's own max - min).

Two of the quantities differ from run to run of ONE build: the slots evaluated wherever rows are drawn from the single-kernel
form's queue (which walker slot a row lands in, and with it the candidates evaluated ahead, goes by timing), and the rounds, which
count what the host had queued beyond a group's last round.  The digest, the calls, the geometry line and the refusals do not.  A
build held against itself shows how often (profiles/walk_host_parity.txt: a sixth of the walks either way)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (40, 2600, 5000, 16384, 40000)
NSTEPS = 9                                              # (>= 8: walks of more rows than walker slots go in two parts)
ROUNDS = [{}, {"RVLL_ROUNDS_GROUPS": "1"}, {"RVLL_ROUNDS_GROUPS": "2", "RVLL_ROUNDS_FORM": "cu"}, {"RVLL_ROUNDS_GROUPS": "4", "RVLL_WALK_SPEC": "1"},
          {"RVLL_ROUNDS_GROUPS": "2"}, {"RVLL_ROUNDS_CHAIN": "1"}, {"RVLL_ROUNDS_PRIO": "1", "RVLL_ROUNDS_W": "16"},
          {"RVLL_WALK_SPEC": "16", "RVLL_ROUNDS_FREE": "100000"}, {"RVLL_ROUNDS_FREE": "1", "RVLL_ROUNDS_DEPTH": "1"},
          {"RVLL_ROUNDS_DEPTH": "9", "RVLL_ROUNDS_PB": "3"}, {"RVLL_ROUNDS_PER": "13700"}]
SINGLE = [{"RVLL_WALK_ROUNDS": "0"}, {"RVLL_WALK_PARTS": "1"}, {"RVLL_WALK_QUEUE": "0"}, {"RVLL_WALK_ROWS": "1"}, {"RVLL_WALK_ROWS": "2"},
          {"RVLL_WALK_ROWS": "3"}, {"RVLL_WALK_FAT": "1"}, {"RVLL_WALK_FIRST": "3"}, {"RVLL_WALK_SPEC": "1"}, {"RVLL_WALK_QUEUE": "8", "RVLL_WALK_ROWS": "1"}]
CHILD_SECONDS = 900


def model_and_start(cfg, K, seed):
    from evidence_amd import GpuRVModel
    from evidence_amd.callbacks import wrapped_params
    from evidence_amd.synthetic import make_workload
    w = make_workload(cfg)
    m = GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict())
    cube = np.random.default_rng(seed).random((2 * K, m.ndim))
    theta, logl = m.prior_loglike_batch(cube)
    lstar = float(np.median(logl))
    keep = np.flatnonzero(logl > lstar)[:K]
    cube, theta, logl = cube[keep], theta[keep], logl[keep]
    d0 = cube - cube.mean(axis=0)
    cov = d0.T @ d0 / (len(cube) - 1)
    if len(cube) <= 2 * m.ndim:                          # too few rows for a full covariance: the variances
        cov = np.diag(np.diag(cov))
    chol = np.linalg.cholesky(cov + 1e-14 * np.eye(m.ndim))
    return m, (cube, theta, logl, lstar, chol, wrapped_params(m.parnames))


class Stderr:
    """fd 2 into a file for as long as the child lives: what the library printed since the last take()"""

    def __init__(self):
        self.file = tempfile.TemporaryFile(mode="w+b")
        os.dup2(self.file.fileno(), 2)
        self.at = 0

    def take(self):
        self.file.seek(self.at)
        text = self.file.read().decode(errors="replace")
        self.at += len(text.encode())
        return text


def child_matrix(cfg):
    """Every walk of cfg's part of the matrix: one JSON line each."""
    err = Stderr()
    os.environ["RVLL_WALK_GEOM_DUMP"] = "1"
    for K in SIZES:
        m, (cube, theta, logl, lstar, chol, wr) = model_and_start(cfg, K, seed=100 * cfg + 7)
        n = len(cube)
        R = 4
        run_start = np.linspace(0, n, R + 1).astype(np.int64)
        runs = dict(run_start=run_start, lstar=np.full(R, lstar), chol=np.broadcast_to(chol, (R,) + chol.shape).copy(), wrapped=wr,
                    seeds=np.arange(11, 11 + R, dtype=np.uint64))
        mixed = np.array([NSTEPS, NSTEPS - 2, NSTEPS, 3], dtype=np.int32)
        with m:
            def walk(name, env, call):
                for k, v in env.items():
                    os.environ[k] = v
                try:
                    res = call()
                    digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in res[:3])).hexdigest()[:20]
                    got = dict(digest=digest, ncalls=np.asarray(res[3]).tolist(), evaluated=m.slice_walk_evaluated(), rounds=m.slice_walk_rounds())
                except Exception as exc:                 # noqa: BLE001  (a walk the library refuses: both builds must refuse it alike)
                    got = dict(error=f"{type(exc).__name__}: {exc}")
                for k in env:
                    del os.environ[k]
                got["geometry"] = [line for line in err.take().splitlines() if line.startswith("[rounds] ")]
                tag = " ".join(f"{k[5:]}={v}" for k, v in env.items()) or "no switch"
                print(json.dumps(dict(name=f"cfg{cfg} K={n:5d} umax={umax:2.0f} {name:12s} {tag}", **got)), flush=True)

            for umax in (30.0, 1.0):
                m.set_slim_table_range(umax)
                chord = lambda: m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=NSTEPS, seed=13)                  # noqa: E731
                walk("chord", {}, chord)
                for env in ROUNDS:
                    walk("chord", dict(RVLL_WALK_ROUNDS="1", **env), chord)
                for env in SINGLE:
                    walk("chord", env, chord)
                stepout = lambda: m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=NSTEPS, seed=13, proposal="stepout")    # noqa: E731
                for env in ({}, {"RVLL_WALK_PARTS": "1"}, {"RVLL_WALK_QUEUE": "0"}, {"RVLL_WALK_ROWS": "1"}):
                    walk("stepout", env, stepout)
                for name, steps in (("runs", NSTEPS), ("runs uniform", np.full(R, NSTEPS, np.int32)), ("runs mixed", mixed)):
                    call = lambda: m.slice_walk_runs(cube, theta, logl, nsteps=steps, **runs)                             # noqa: E731,B023
                    for env in ({}, {"RVLL_WALK_ROUNDS": "1"}, {"RVLL_WALK_ROUNDS": "0"}, {"RVLL_WALK_PARTS": "1"}, {"RVLL_WALK_ROWS": "1"}):
                        walk(name, env, call)
                call = lambda: m.slice_walk_runs(cube, theta, logl, nsteps=mixed, proposal="stepout", **runs)                 # noqa: E731
                walk("runs stepout", {}, call)


def child_time():
    """calls / s inside the walk call at bench.py's nested configuration (cfg3, nsteps = 3 ndim): one JSON line a size."""
    for K in (2600, 16384, 40000):                       # single kernel, rounds, two parts
        m, (cube, theta, logl, lstar, chol, wr) = model_and_start(3, K, seed=5)
        with m:
            nsteps = 3 * m.ndim
            m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=nsteps, seed=1)              # warm-up
            calls = seconds = 0
            for seed in (2, 3, 4):
                t0 = time.perf_counter()
                res = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=nsteps, seed=seed)
                seconds += time.perf_counter() - t0
                calls += int(res[3])
            print(json.dumps(dict(K=K, rate=calls / seconds, rounds=m.slice_walk_rounds())), flush=True)


def fail(text):
    print(text, flush=True)
    sys.exit(3)


def run_child(library, what):
    """The JSON lines of `what` through `library` (None: this tree's) in a fresh process; exits when the child fails."""
    env = dict(os.environ)
    env.pop("RVLL_LIBRARY", None)
    if library:
        env["RVLL_LIBRARY"] = os.path.abspath(library)
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what], env=env, stdout=subprocess.PIPE,
                              timeout=CHILD_SECONDS, text=True)
    except subprocess.TimeoutExpired:
        fail(f"FAILED: {what} through {library or 'this build'} did not end in {CHILD_SECONDS} s")
    if done.returncode != 0:
        fail(f"FAILED: {what} through {library or 'this build'} ended with status {done.returncode}\n{done.stdout[-2000:]}")
    return [json.loads(line) for line in done.stdout.splitlines() if line.startswith("{")]


def matrix(earlier, mine, keep_going):
    total = different = 0
    by_field = {}
    for cfg in (1, 3, 5):
        old, new = run_child(earlier, f"matrix{cfg}"), run_child(mine, f"matrix{cfg}")
        if len(old) != len(new):
            fail(f"DIFFERENT: cfg{cfg}: {len(old)} / {len(new)} walks")
        for a, b in zip(old, new):
            same = a == b
            what = a["error"] if "error" in a else (f"{a['digest']} calls {np.sum(a['ncalls'])} evaluated {a['evaluated']} rounds {a['rounds']}"
                                                    + (" | " + a["geometry"][0][9:] if a["geometry"] else ""))
            print(f"{a['name']:75s} {'equal' if same else 'DIFFERENT'}   {what}", flush=True)
            total += 1
            if not same:
                different += 1
                fields = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
                for k in fields:
                    by_field[k] = by_field.get(k, 0) + 1
                print("    earlier / new: " + "; ".join(f"{k} {a.get(k)} / {b.get(k)}" for k in fields), flush=True)
                if not keep_going:
                    sys.exit(1)
    if different:
        print(f"DIFFERENT: {different} of {total} walks (" + ", ".join(f"{k}: {n}" for k, n in sorted(by_field.items())) + ")")
        sys.exit(1)
    print(f"all equal: {total} walks, digest of cube / theta / log-L, calls, slots evaluated, rounds and the [rounds] geometry line")


def timing(earlier, mine, repeats):
    rates = {}
    for _ in range(repeats):
        for who, library in (("earlier", earlier), ("new", mine)):
            for got in run_child(library, "time"):
                rates.setdefault((got["K"], got["rounds"] > 0), {"earlier": [], "new": []})[who].append(got["rate"])
    ok = True
    for (K, by_rounds), r in sorted(rates.items()):
        name = f"cfg3 K={K} nsteps=57 ({'rounds' if by_rounds else 'single kernel'})"
        for who in ("earlier", "new"):
            print(f"{name:45s} {who:8s} calls/s inside the walk: " + "  ".join(f"{v:.4e}" for v in r[who]) + f"   median {np.median(r[who]):.4e}")
        spread = max(r["earlier"]) - min(r["earlier"])
        short = np.median(r["earlier"]) - np.median(r["new"])
        fine = len(r["new"]) == len(r["earlier"]) == repeats and short <= spread
        ok = ok and fine
        print(f"{name:45s} new median below the earlier one by {short:.3e}, allowed {spread:.3e} (its max - min): {'ok' if fine else 'SLOWER'}",
              flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("earlier", nargs="?", help="librvll.so of the earlier commit, built outside this tree")
    ap.add_argument("new", nargs="?", help="the library held against it (default: this tree's)")
    ap.add_argument("--keep-going", action="store_true", help="list every difference before exiting")
    ap.add_argument("--time", action="store_true", help="calls per second inside the walk, both libraries alternately")
    ap.add_argument("--repeats", type=int, default=5, help="--time: processes a library (at least five)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child_time() if args.child == "time" else child_matrix(int(args.child[len("matrix"):]))
    elif not args.earlier or not os.path.isfile(args.earlier):
        ap.error("the earlier library is missing")
    elif args.time:
        timing(args.earlier, args.new, max(5, args.repeats))
    else:
        matrix(args.earlier, args.new, args.keep_going)
