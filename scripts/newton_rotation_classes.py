#!/usr/bin/env python3
"""How would eccentricity classes split the waves between a short rotation, a middle one and the full sin / cos?  (CPU only, numpy.)

From its second evaluation on a Newton solve takes (sin, cos) at E + h with the pair at E in registers.  A rule by classes
picks, per lane, a short series (|h| <= 2^-6, e <= kEccShort), the minimax kernels on h (|h| <= pi/4, e <= 0.6) or the full
sincos, and the classes exist only to keep the lanes of a wave on ONE of the three.  This prints, under a BASELINE config's
priors,

  * per eccentricity bin, the share of second-and-later steps with |h| <= 2^-6 and of first steps with |h| <= pi/4, and
    the largest kEccShort for which 99 % of the second-and-later steps of all planets at or below it are short;
  * for a few kEccShort, with the short series allowed from the second or only from the third evaluation on, what a wave (64
    consecutive (point, epoch) items) executes: the share of wave-level evaluations that run one, two or three of the paths,
    and the vector instructions of the pair per wave solve against the full pair every trip.

The model counts vector instructions only.  On the MI355X the per-lane choice itself — mask arithmetic and two branches a
trip — cost more than every variant of it saved, and what the kernels ship is the middle rotation for every lane with the full
routine behind an unlikely branch (rvll_math.h, newton_next_sincos; profiles/r05_newton_rotation.txt holds both).

    python scripts/newton_rotation_classes.py [--config 3] [--points 2048]
"""
import argparse
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from evidence_amd.synthetic import make_workload  # noqa: E402

FULL, MID, SHORT = 30, 19, 12          # vector instructions of the pair: reduction + quadrant + kernels; rotate_mid; rotate_short
H_SHORT, H_MID, ECC_MID = 2.0 ** -6, math.pi / 4, 0.6
TOL, SAFE = 1e-4, 8


def solves(w, points):
    """(M, e) of every (planet, point, epoch) item in the order the tile forms its waves: (planet, wave, lane)."""
    th = w.sample_theta(points, seed=1234)
    t = w.table.time
    names = list(w.parnames)
    planets = sorted({n.split("_")[0] for n in names if n.startswith("planet")})
    Ms, es = [], []
    rng = np.random.default_rng(1)
    for p in planets:
        P = th[:, names.index(f"{p}_period")][:, None]
        e = np.minimum(th[:, names.index(f"{p}_ecc")], 0.99)[:, None]
        M = (2 * np.pi / P * (t[None, :] - t[0]) + rng.uniform(0, 2 * np.pi, (len(th), 1))).reshape(-1)
        ee = np.broadcast_to(e, (len(th), len(t))).reshape(-1)
        n = (M.size // 64) * 64
        Ms.append(M[:n].reshape(-1, 64))
        es.append(ee[:n].reshape(-1, 64))
    return np.concatenate(Ms), np.concatenate(es)


def run(M, e):
    """|h| in front of every evaluation, per trip: list of (active mask, |h|) — trip 0 is the evaluation at E = M."""
    E = M.copy()
    active = np.ones(M.shape, bool)
    prev = np.full(M.shape, np.inf)
    trips = []
    for _ in range(SAFE):
        if not active.any():
            break
        trips.append((active.copy(), prev.copy()))
        dE = -(E - e * np.sin(E) - M) / (1 - e * np.cos(E))
        E = np.where(active, E + dE, E)
        prev = np.where(active, np.abs(dE), prev)
        active &= np.abs(dE) > TOL
    return trips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--points", type=int, default=2048)
    args = ap.parse_args()
    w = make_workload(args.config)
    M, e = solves(w, args.points)
    trips = run(M, e)
    print(f"cfg{args.config}: {M.size} solves in {M.shape[0]} waves; wave-level evaluations per solve "
          f"{sum(a.any(axis=1).sum() for a, _ in trips) / M.shape[0]:.3f}")

    edges = np.array([0, .05, .1, .15, .2, .25, .3, .35, .4, .5, .6, .7, .8, .9, 1.0])
    later_n = np.zeros(len(edges) - 1)
    later_short = np.zeros(len(edges) - 1)
    first_n = np.zeros(len(edges) - 1)
    first_mid = np.zeros(len(edges) - 1)
    for k, (a, h) in enumerate(trips[1:], 1):
        b = np.digitize(e[a], edges) - 1
        if k == 1:
            first_n += np.bincount(b, minlength=len(later_n))
            first_mid += np.bincount(b, weights=(h[a] <= H_MID), minlength=len(later_n))
        else:
            later_n += np.bincount(b, minlength=len(later_n))
            later_short += np.bincount(b, weights=(h[a] <= H_SHORT), minlength=len(later_n))
    print("  e bin          first steps |h| <= pi/4     second-and-later steps |h| <= 2^-6    (cumulative from e = 0)")
    cn = np.cumsum(later_n)
    cs = np.cumsum(later_short)
    for i in range(len(later_n)):
        print(f"  [{edges[i]:.2f}, {edges[i + 1]:.2f})   {100 * first_mid[i] / max(first_n[i], 1):8.3f} %"
              f"                 {100 * later_short[i] / max(later_n[i], 1):8.3f} %"
              f"                    {100 * cs[i] / max(cn[i], 1):8.3f} %")
    # the largest bound with >= 99 % of the second-and-later steps at or below it short (per-planet eccentricity, 0.01 grid)
    la = np.concatenate([e[a] for a, _ in trips[2:]])
    lh = np.concatenate([h[a] for a, h in trips[2:]])
    best = 0.0
    for b in np.arange(0.01, 0.99, 0.01):
        m = la <= b
        if m.any() and np.mean(lh[m] <= H_SHORT) >= 0.99:
            best = b
    print(f"  largest kEccShort with >= 99 % of the second-and-later steps of planets at or below it short: {best:.2f}")

    base = sum(a.any(axis=1).sum() for a, _ in trips) * FULL
    print("  kEccShort   evaluations running 1 / 2 / 3 paths      pair instructions per wave solve (full pair every trip: "
          f"{base / M.shape[0]:.1f})")
    for ks, from_trip in [(k, f) for f in (1, 2) for k in (0.15, 0.2, 0.25, 0.3, 0.35, 0.4)]:
        cost = 0
        npaths = np.zeros(4)
        for k, (a, h) in enumerate(trips):
            sh = a & (e <= ks) & (h <= H_SHORT) & (k >= from_trip)
            md = a & ~sh & (e <= ECC_MID) & (h <= H_MID)
            fu = a & ~sh & ~md
            ws, wm, wf = sh.any(axis=1), md.any(axis=1), fu.any(axis=1)
            cost += ws.sum() * SHORT + wm.sum() * MID + wf.sum() * FULL
            npaths += np.bincount(ws.astype(int) + wm + wf, minlength=4)
        tot = npaths[1:].sum()
        print(f"  {ks:.2f} (short from evaluation {from_trip + 1})   {100 * npaths[1] / tot:5.1f} / {100 * npaths[2] / tot:5.1f} / {100 * npaths[3] / tot:5.1f} %"
              f"                     {cost / M.shape[0]:.1f}  ({100 * (cost - base) / base:+.1f} % of the pair's)")


if __name__ == "__main__":
    main()
