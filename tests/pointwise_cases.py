"""Inputs in which every merged row counts, and the comparison of a pointwise result with the numpy definition: shared by
tests/test_pointwise_cases_host.py (are the inputs what the GPU tests need, does the comparison refuse a wrong result?),
tests/test_gpu_pointwise.py and tests/test_gpu_pointwise_tiles.py (the device against the definition at every cut of the product's
geometry: 64 replicates and 64 columns a workgroup, 16384 rows a slab, 64 rows a staged chunk with a 16-row look-ahead, the block
of replicates of the shared driver).

A sampler-shaped run gives its first rows a weight of e^-hundreds, so a product that skipped a chunk of them would pass any bound.
flat_run makes a run whose expected weights are flat, marker_table a table in which every row sits at least about 0.5 from the
weighted mean; together, leaving any row, k-step, 16-row group or chunk out of the sums moves mean or var by far more than the
bounds below (tests/test_pointwise_cases_host.py holds that to a factor of 100 for every shape the GPU tests use).

Bounds of compare (derived in tests/test_gpu_pointwise.py's docstring, none from a measurement).  With z = t - a and, from the
definition's weights, S1 = sum p |z| / P, M1 = sum p z / P, M2 = sum p z^2 / P:
    |lpd err| <= 2.5e-10          |loo err| <= 2.5e-10
    |mean err| <= 1e-10 S1        |var err| <= 2e-10 (M2 + 2 |M1| S1)"""
import numpy as np

from evidence_amd import merge, pointwise

KEYS = ("lpd", "loo", "mean", "var")
CONSTANT = -3.25                         # the value of marker_table's constant column
EMPTY = (np.empty(0), np.empty(0))       # a run without rows: something for the bootstrap to draw besides the one run
FACTOR = 100.0                           # what leaving rows out has to move an output by, in bounds of that output
CHUNK_MASS = 1e-5                        # what every full chunk holds of a random-mode replicate's mass, at least
CHUNK, GROUP, KSTEP = 64, 16, 4          # rows of a staged chunk, of the operand's look-ahead, of one matrix instruction


SEED = 20                                # of the replicates, in every test
SMALL = (130, 8)                        # rows and live points of the run of the replicate, block and column tests
REP_COUNTS = (63, 64, 65, 128, 129, 130)
BLOCK_REPS = (150, 70)                   # replicates of a call and of its blocks: 70, 70 and 10, each across a tile edge
WIDE_REPS = 65
WIDE_UNITS = (15, 16, 31, 32, 48)        # 61 | 65, 125 | 129 and 193 columns
LIMIT_UNITS = (4096, 4097)               # the most units of one device call (257 column tiles), and one more
ROW_EDGES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129)


def slab_edges(slab):
    return (slab - 1, slab, slab + 1, 2 * slab, 2 * slab + 1)


def shapes(slab):
    """(rows, live points, units) of every input of tests/test_gpu_pointwise_tiles.py."""
    out = [SMALL + (3,)] + [SMALL + (u,) for u in WIDE_UNITS + LIMIT_UNITS]
    out += [(n, max(1, n // 16), 3) for n in ROW_EDGES] + [(n, n // 80, 3) for n in slab_edges(slab)]
    return out


def layout(units):
    """(constant, twin) of a table of `units` units: of three, the middle one is constant; wider ones have the constant in the
    middle and twins one from either end — in different 64-column tiles of the operand (4 units + 1 columns) from 31 units on."""
    return (1, None) if units == 3 else (units // 2, (1, units - 2))


def case(n, nlive, units, pad=0):
    """(table, logl, birth, run_start) of the shape: flat_run and marker_table seeded by the shape, with `pad` empty runs after
    the one run."""
    constant, twin = layout(units)
    logl, birth, run_start = arrays([flat_run(n, nlive, n)] + [EMPTY] * pad)
    return marker_table(n, units, n + units, constant, twin), logl, birth, run_start


def flat_run(n, nlive, seed):
    """(logl, birth) of one run of n rows whose expected weights are flat: logl_i = i / nlive, born from -inf for i < nlive and on
    logl_{i - nlive} after, so nlive points are live until the last nlive rows and L X stays put; the rows are then permuted (a
    run's rows come in any order)."""
    n, nlive = int(n), int(nlive)
    logl = np.arange(n, dtype=np.float64) / nlive
    birth = np.full(n, -np.inf)
    if n > nlive:
        birth[nlive:] = logl[:n - nlive]
    perm = np.random.default_rng(seed).permutation(n)
    return logl[perm], birth[perm]


def arrays(runs):
    logl = np.concatenate([r[0] for r in runs])
    birth = np.concatenate([r[1] for r in runs])
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int64)
    return logl, birth, run_start


def marker_table(n, units, seed, constant=None, twin=None):
    """[n, units]: every column drawn on its own with sizes in [1, 2] and random signs, so that every row is at least about 0.5
    from any weighted mean of its column.  constant: the index of a column that is CONSTANT in every row (the kernel promises it
    is exact); twin = (u, v): column v is a copy of column u (their results must agree bit for bit wherever the two sit)."""
    rng = np.random.default_rng(1000 + seed)
    t = rng.uniform(1.0, 2.0, (int(n), int(units))) * rng.choice([-1.0, 1.0], (int(n), int(units)))
    if twin is not None:
        t[:, twin[1]] = t[:, twin[0]]
    if constant is not None:
        t[:, constant] = CONSTANT
    return t


def sizes(table, logl, birth, run_start, shifts, nrep, **kw):
    """S1, |M1| and M2 [nrep, U] from the definition's weights."""
    logwt = merge.replicates_arrays(logl, birth, run_start, nrep, return_logwt=True, **kw)[2]
    z = table[merge.merge_arrays(logl, birth, run_start)["order"]] - shifts[2]
    with np.errstate(invalid="ignore"):
        p = np.exp(logwt)
    p = p / p.sum(axis=1, keepdims=True)
    return p @ np.abs(z), np.abs(p @ z), p @ (z * z)


def bounds(s1, m1, m2):
    return dict(lpd=np.full_like(s1, 2.5e-10), loo=np.full_like(s1, 2.5e-10), mean=1e-10 * s1, var=2e-10 * (m2 + 2.0 * m1 * s1))


def compare(got, ref, sz):
    """The replicates of the result dict `got` (its first ones, when it has more than `ref`) against the definition's dict `ref`
    within the bounds of the module docstring, sz = sizes(...) of the same call; every replicate and every unit.  A replicate
    without mass is NaN in all four outputs on both sides, every other entry is finite.  Returns (bounds, largest error over its
    bound per output)."""
    nrep = ref["logz"].shape[0]
    assert np.array_equal(ref["shifts"], got["shifts"]) and np.array_equal(ref["truncated_rows"], got["truncated_rows"])
    assert np.array_equal(ref["loo_ess"], got["loo_ess"])
    bound = bounds(*sz)
    empty = np.isneginf(ref["logz"])
    assert np.array_equal(np.isneginf(got["logz"][:nrep]), empty)
    live = ~empty
    close = np.abs(got["logz"][:nrep][live] - ref["logz"][live]) <= 1e-12 * np.maximum(1.0, np.abs(ref["logz"][live]))
    assert np.all(close)
    worst = {}
    for key in KEYS:
        out = got[key][:nrep]
        assert out.shape == ref[key].shape == bound[key].shape, key
        assert np.all(np.isnan(out[empty])) and np.all(np.isnan(ref[key][empty])), key
        assert np.all(np.isfinite(out[live])) and np.all(np.isfinite(ref[key][live])), key
        err = np.abs(out[live] - ref[key][live])
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err > 0, err / bound[key][live], 0.0)
        worst[key] = float(ratio.max()) if ratio.size else 0.0
    print("largest error over its bound:", worst)
    for key in KEYS:
        assert worst[key] <= 1.0, (key, worst[key])
    assert np.array_equal(got["waic"], got["lpd"] - got["var"], equal_nan=True)
    return bound, worst


def check(dev, table, logl, birth, run_start, nrep, unit_block=None, **kw):
    """The first nrep replicates of the device result `dev` against the definition (in blocks of unit_block units: the same
    bits in less memory); returns (bounds, the definition's dict)."""
    ref = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=nrep, unit_block=unit_block, **kw)
    bound, _ = compare(dev, ref, sizes(table, logl, birth, run_start, ref["shifts"], nrep, **kw))
    return bound, ref


def same_bits(a, b, keys=KEYS + ("waic", "logz", "information")):
    """Two result dicts agree bit for bit (NaN equal to NaN) in `keys`."""
    for key in keys:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def weights(logl, birth, run_start, nrep, **kw):
    """p [nrep, N] in merged order as the definition forms it: exp(logwt) of merge.replicates_arrays."""
    with np.errstate(invalid="ignore", under="ignore"):
        return np.exp(merge.replicates_arrays(logl, birth, run_start, nrep, return_logwt=True, **kw)[2])


def reduced(ref, table, logl, birth, run_start, p):
    """A copy of the definition's dict `ref` whose four outputs (and waic) are the definition's own reduction (pointwise.operand,
    pointwise._reduce) of the weights p [S, N] in merged order: with p = weights(...) the bits of `ref`, with some of p set to
    zero what a product that left those rows out would return."""
    order = merge.merge_arrays(logl, birth, run_start)["order"]
    shifts = ref["shifts"]
    bt = pointwise.operand(table[order], shifts)
    out = dict(ref)
    for key in KEYS:
        out[key] = np.empty_like(ref[key])
    for s in range(p.shape[0]):
        pointwise._reduce(p[s], bt, shifts, *(out[key][s] for key in KEYS))
    out["waic"] = out["lpd"] - out["var"]
    return out


def replaced(ref, **outputs):
    """A copy of the dict `ref` with the given outputs, and the waic that goes with them."""
    out = dict(ref, **outputs)
    out["waic"] = out["lpd"] - out["var"]
    return out


def moved(p, z, width):
    """For the weights p [N] of one replicate and z = t - a [N, U] in merged order: how far leaving out the rows
    [j width, (j + 1) width) moves mean or var, in bounds of that output (the larger of the two), float [groups, U].  Leaving out
    all the mass leaves NaN, which compare refuses: infinity here.  A unit whose z is zero in every row (a constant column) has
    bounds of zero and moves by zero: NaN here."""
    p = p / p.sum()
    starts = np.arange(0, p.shape[0], width)
    s1, m1, m2 = p @ np.abs(z), p @ z, p @ (z * z)
    bound = bounds(s1, np.abs(m1), m2)
    gp = np.add.reduceat(p, starts)[:, None]
    gz = np.add.reduceat(p[:, None] * z, starts, axis=0)
    gzz = np.add.reduceat(p[:, None] * z * z, starts, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n1, n2 = (m1 - gz) / (1.0 - gp), (m2 - gzz) / (1.0 - gp)
        by = np.maximum(np.abs(n1 - m1) / bound["mean"], np.abs((n2 - n1 * n1) - (m2 - m1 * m1)) / bound["var"])
    return np.where(np.broadcast_to(gp >= 1.0, by.shape), np.inf, by)


def slab_edge_rows(n, slab):
    """The rows (merged order) next to the slab edges of a run of n rows: the first and the last row of the first and of the last
    chunk of every slab (the last chunk of the last slab may be a part of one), the slab's own first and last row among them."""
    rows = set()
    for begin in range(0, n, slab):
        end = min(begin + slab, n)
        rows.update((begin, min(begin + CHUNK, end) - 1, (end - 1) // CHUNK * CHUNK, end - 1))
    return sorted(rows)
