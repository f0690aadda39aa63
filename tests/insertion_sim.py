"""A simulated nested sampler on a one-dimensional problem whose constrained prior is known exactly (the insertion-index tests).

The prior is uniform u in (0, 1) and log-L = -u, so the region L > L* is u < u* = -L*.  Every iteration kills the kbatch lowest
live points and draws kbatch replacements uniformly from u < reach(it) u* — reach 1 is a perfect sampler, reach < 1 one that
cannot get near the contour.  Rows: the dead points in death order, then the final live points, as the drivers give them.
`ranks` is what the simulation records at insertion time: each new point's rank among the nlive live points right after its
batch was inserted (-1 for the initial points)."""
import numpy as np


def simulate(nlive, kbatch, niter, seed, reach=None):
    rng = np.random.default_rng(seed)
    reach = reach or (lambda it: 1.0)
    logl = -rng.random(nlive)
    birth = np.full(nlive, -np.inf)
    rank = np.full(nlive, -1, dtype=np.int64)
    dead_l, dead_b, dead_r = [], [], []
    for it in range(niter):
        order = np.argsort(logl, kind="stable")
        dead = order[:kbatch]
        lstar = logl[dead[-1]]
        dead_l.append(logl[dead]); dead_b.append(birth[dead]); dead_r.append(rank[dead])
        logl[dead] = -(-lstar) * reach(it) * rng.random(kbatch)
        birth[dead] = lstar
        for i in dead:
            rank[i] = np.count_nonzero(logl < logl[i])
    return (np.concatenate(dead_l + [logl]), np.concatenate(dead_b + [birth]), np.concatenate(dead_r + [rank]))
