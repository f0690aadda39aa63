"""CPU: the inputs and the comparison of tests/pointwise_cases.py, on the numpy definition alone.  What gives
tests/test_gpu_pointwise_tiles.py its teeth is checked here, for every (rows, units) it uses:
- the expected weights of flat_run are flat (every row at least 0.96 / n of the mass);
- with mode="expected" and no bootstrap, leaving any one row, 4-row k-step, 16-row group or 64-row chunk of the merged order out
  of the sums moves mean or var of every marker unit by at least 100 bounds of that output — every row and every group of every
  shape in closed form, and the rows next to the slab edges once more by setting their weight to zero and reducing again with the
  definition's own code, which compare then refuses;
- with mode="random" every full 64-row chunk holds at least 1e-5 of the mass of every replicate (a single row may hold 1e-10 of
  it there, and so may the part of a chunk at the run's end: those rows are what the expected-mode condition is for);
- compare raises on the definition's own result with two replicates swapped, replicate 64 replaced by replicate 0, the last row
  dropped, the first chunk of the second slab dropped, the units of the second column tile shifted by one.
These are conditions on the inputs, not measurements: an input that fails one is changed, the factors are not."""
import numpy as np
import pytest

from evidence_amd import merge, pointwise
import pointwise_cases as pc

EXPECTED = dict(seed=pc.SEED, mode="expected", bootstrap=False)


def _groups(slab):
    every = pc.shapes(slab)
    return dict(small=every[:1], wide=every[1:1 + len(pc.WIDE_UNITS)], limit=every[6:8], rows=every[8:8 + len(pc.ROW_EDGES)],
                slabs=every[-5:])


def test_the_shapes_sit_on_both_sides_of_every_cut():
    slab = pointwise.slab_rows()
    g = _groups(slab)
    assert sum(len(v) for v in g.values()) == len(pc.shapes(slab)) == 1 + 5 + 2 + 14 + 5
    assert g["small"] == [(130, 8, 3)] and [s[2] for s in g["wide"]] == [15, 16, 31, 32, 48]
    assert [4 * s[2] + 1 for s in g["wide"]] == [61, 65, 125, 129, 193] and [s[2] for s in g["limit"]] == [4096, 4097]
    assert [s[0] for s in g["rows"]] == [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129]
    assert [s[0] for s in g["slabs"]] == [slab - 1, slab, slab + 1, 2 * slab, 2 * slab + 1]
    assert all(s[1] == max(1, s[0] // 16) for s in g["rows"]) and all(s[1] == s[0] // 80 for s in g["slabs"])
    assert pointwise.MAX_UNITS == 4096
    for units in pc.WIDE_UNITS[2:] + pc.LIMIT_UNITS:                       # the twins sit in different column tiles
        u, v = pc.layout(units)[1]
        assert (1 + 4 * u) // 64 != (1 + 4 * v) // 64


def test_flat_run_and_marker_table_are_what_they_say():
    logl, birth = pc.flat_run(130, 8, 3)
    order = np.argsort(logl)
    assert np.array_equal(logl[order], np.arange(130) / 8) and np.all(np.isneginf(birth[order][:8]))
    assert np.array_equal(birth[order][8:], logl[order][:-8]) and not np.array_equal(order, np.arange(130))
    t = pc.marker_table(130, 9, 3, constant=4, twin=(1, 7))
    assert np.all(t[:, 4] == pc.CONSTANT) and np.array_equal(t[:, 1], t[:, 7])
    rest = np.abs(np.delete(t, 4, axis=1))
    assert rest.min() >= 1.0 and rest.max() <= 2.0 and np.unique(np.delete(t, [4, 7], axis=1)).size == 130 * 7
    assert (t[:, 0] > 0).sum() > 30 and (t[:, 0] < 0).sum() > 30


@pytest.mark.parametrize("group", ["small", "wide", "limit", "rows", "slabs", "large"])
def test_the_expected_weights_are_flat(group):
    shapes = [(32769, 400, 3), (16385, 200, 3), (130, 8, 3)] if group == "large" else _groups(pointwise.slab_rows())[group]
    for n, nlive, _ in shapes:
        logl, birth, run_start = pc.arrays([pc.flat_run(n, nlive, n)])
        w = np.exp(merge.merge_arrays(logl, birth, run_start)["logwt"])
        assert w.min() >= 0.96 / n * w.sum(), (n, nlive, w.min() * n / w.sum())


@pytest.mark.parametrize("group", ["small", "wide", "limit", "rows", "slabs"])
def test_leaving_out_any_row_kstep_group_or_chunk_moves_mean_or_var_by_100_bounds(group):
    slab = pointwise.slab_rows()
    least = np.inf
    for n, nlive, units in _groups(slab)[group]:
        table, logl, birth, run_start = pc.case(n, nlive, units)
        constant = pc.layout(units)[0]
        markers = np.arange(units) != constant
        ref = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=1, **EXPECTED)
        p = pc.weights(logl, birth, run_start, 1, **EXPECTED)
        z = table[merge.merge_arrays(logl, birth, run_start)["order"]] - ref["shifts"][2]
        assert np.all(z[:, constant] == 0.0)
        for width in (1, pc.KSTEP, pc.GROUP, pc.CHUNK):
            by = pc.moved(p[0], z, width)
            assert by.shape == (-(-n // width), units) and np.all(np.isnan(by[:, constant]) | (n <= width))
            assert np.all(by[:, markers] >= pc.FACTOR), (n, units, width, by[:, markers].min())
            least = min(least, by[:, markers].min())
        if units != 3:
            continue
        # once more with the definition's own reduction, a row at a time: all of them on the small runs, the slab edges' on the large
        assert np.array_equal(pc.reduced(ref, table, logl, birth, run_start, p)["mean"], ref["mean"])
        sz = pc.sizes(table, logl, birth, run_start, ref["shifts"], 1, **EXPECTED)
        bound = pc.bounds(*sz)
        pc.compare(ref, ref, sz)
        rows = range(n) if n <= 130 else pc.slab_edge_rows(n, slab)
        if n > 130:
            assert {0, 63, slab - 64, n - 1, (n - 1) // 64 * 64} <= set(rows)
            assert n < slab or slab - 1 in rows
            assert n <= slab or {slab, min(slab + 63, n - 1)} <= set(rows)
            assert n < 2 * slab or {2 * slab - 64, 2 * slab - 1} <= set(rows)
        for r in rows:
            q = p.copy()
            q[0, r] = 0.0
            out = pc.reduced(ref, table, logl, birth, run_start, q)
            with np.errstate(invalid="ignore", divide="ignore"):
                by = np.maximum(np.abs(out["mean"] - ref["mean"]) / bound["mean"], np.abs(out["var"] - ref["var"]) / bound["var"])
            assert np.all(np.isnan(out["mean"])) if n == 1 else np.all(by[0, markers] >= pc.FACTOR), (n, r, by)
            with pytest.raises(AssertionError):
                pc.compare(out, ref, sz)
    print(group, ": the least move, in bounds:", least)


@pytest.mark.parametrize("group", ["small", "rows", "slabs"])
def test_every_full_chunk_holds_mass_in_every_random_replicate(group):
    slab = pointwise.slab_rows()
    least = np.inf
    for n, nlive, units in _groups(slab)[group]:
        for bootstrap in ((False, True) if group == "small" else (False,)):
            pad, nrep = (2, max(pc.REP_COUNTS)) if group == "small" else (0, pc.WIDE_REPS)
            _, logl, birth, run_start = pc.case(n, nlive, units, pad)
            p = pc.weights(logl, birth, run_start, nrep, seed=pc.SEED, mode="random", bootstrap=bootstrap)
            total = p.sum(axis=1)
            live = total > 0
            assert live.all() != bootstrap and live.sum() > nrep // 2
            full = n // pc.CHUNK
            if full == 0:
                continue
            mass = p[live, :full * pc.CHUNK].reshape(live.sum(), full, pc.CHUNK).sum(axis=2) / total[live, None]
            assert mass.min() >= pc.CHUNK_MASS, (n, bootstrap, mass.min())
            least = min(least, mass.min())
    print(group, ": the least mass of a full chunk:", least)


def _refused(out, ref, sz):
    with pytest.raises(AssertionError):
        pc.compare(out, ref, sz)


def test_compare_refuses_swapped_replicates_and_shifted_units():
    """The run and the replicate count of the column-tile tests, 32 units: columns 64 .. 127 of the operand, the second column
    tile, are the last column of unit 15, units 16 .. 30 and three columns of unit 31."""
    table, logl, birth, run_start = pc.case(*pc.SMALL, 32)
    kw = dict(seed=pc.SEED, mode="random", bootstrap=False)
    ref = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=pc.WIDE_REPS, **kw)
    sz = pc.sizes(table, logl, birth, run_start, ref["shifts"], pc.WIDE_REPS, **kw)
    pc.compare(ref, ref, sz)
    pc.compare(pc.replaced(ref), ref, sz)
    assert np.array_equal(pc.reduced(ref, table, logl, birth, run_start, pc.weights(logl, birth, run_start, pc.WIDE_REPS, **kw))["var"],
                          ref["var"])
    swapped, first_again, shifted = ({k: ref[k].copy() for k in pc.KEYS} for _ in range(3))
    for k in pc.KEYS:
        swapped[k][[3, 4]] = ref[k][[4, 3]]
        first_again[k][64] = ref[k][0]
        shifted[k][:, 16:31] = ref[k][:, 17:32]
    for out in (swapped, first_again, shifted):
        _refused(pc.replaced(ref, **out), ref, sz)
        for k in pc.KEYS:                                                   # each output on its own is enough
            _refused(pc.replaced(ref, **{k: out[k]}), ref, sz)
    # a NaN where the definition has a number, which no error bound sees
    for k in pc.KEYS:
        holed = ref[k].copy()
        holed[64, 31] = np.nan
        _refused(pc.replaced(ref, **{k: holed}), ref, sz)


@pytest.mark.parametrize("mode", ["expected", "random"])
def test_compare_refuses_a_dropped_last_row_and_a_dropped_chunk_of_the_second_slab(mode):
    slab = pointwise.slab_rows()
    n = 2 * slab + 1
    table, logl, birth, run_start = pc.case(n, n // 80, 3)
    kw = dict(seed=pc.SEED, mode=mode, bootstrap=False)
    nrep = 3
    ref = pointwise.pointwise_arrays(table, logl, birth, run_start, nsamples=nrep, **kw)
    sz = pc.sizes(table, logl, birth, run_start, ref["shifts"], nrep, **kw)
    p = pc.weights(logl, birth, run_start, nrep, **kw)
    same = pc.reduced(ref, table, logl, birth, run_start, p)
    for k in pc.KEYS + ("waic",):
        assert np.array_equal(same[k], ref[k]), k
    pc.compare(same, ref, sz)
    chunk = p.copy()
    chunk[:, slab:slab + pc.CHUNK] = 0.0
    _refused(pc.reduced(ref, table, logl, birth, run_start, chunk), ref, sz)
    if mode == "expected":                                                  # a single row may weigh next to nothing in random mode
        last = p.copy()
        last[:, -1] = 0.0
        _refused(pc.reduced(ref, table, logl, birth, run_start, last), ref, sz)
        small = pc.case(*pc.SMALL, 3)
        ref = pointwise.pointwise_arrays(*small, nsamples=nrep, **kw)
        last = pc.weights(*small[1:], nrep, **kw)
        last[:, -1] = 0.0
        _refused(pc.reduced(ref, *small, last), ref, pc.sizes(*small, ref["shifts"], nrep, **kw))
