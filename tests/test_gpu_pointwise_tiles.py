"""The matrix-unit product of the pointwise checks (csrc/rvll_pointwise.hip: product_kernel, finish_kernel) on both sides of every
cut of its geometry, against the numpy definition of evidence_amd/pointwise.py on every replicate and every unit:
- 64 replicates a workgroup: 63 | 64 | 65 and 128 | 129 | 130 replicates in one block, a second and a third tile in grid z;
- the blocks of the shared driver: 150 replicates in blocks of 70, 70 and 10, each across a tile edge and behind a non-zero s0;
- 64 columns a workgroup: 61 | 65, 125 | 129 and 193 columns, and the 4096 units (257 column tiles) that one call takes;
- 64 rows a staged chunk with a 16-row look-ahead on the operand: 1 to 5, 15 | 16 | 17, 63 | 64 | 65 and 127 | 128 | 129 rows;
- 16384 rows a slab: one row short of one slab, one slab, one row more, two slabs, two slabs and a row.
The inputs are tests/pointwise_cases.py's: a run whose expected weights are flat and a table in which every row is a marker, so
that a row, a k-step, a 16-row group or a chunk left out anywhere is a hundred bounds or more (tests/
test_pointwise_cases_host.py).  The bounds are those of tests/test_gpu_pointwise.py, unchanged; the largest ratios are printed.
Where a claim is about bits it is np.array_equal with NaN equal to NaN: a replicate's bits depend on its weights, the column
and the slab cut, not on the slot in a tile, the tile, the block or the units beside it."""
import numpy as np
import pytest

from evidence_amd import pointwise
import pointwise_cases as pc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROWS = ("lpd", "loo", "mean", "var", "waic")


def _device(case, nsamples, **kw):
    return pointwise.pointwise_arrays(*case, nsamples=nsamples, seed=pc.SEED, device=0, **kw)


def _unit(case, u):
    return (np.ascontiguousarray(case[0][:, u:u + 1]),) + tuple(case[1:])


def _same_unit(wide, u, alone):
    for key in ROWS:
        assert np.array_equal(wide[key][:, u], alone[key][:, 0], equal_nan=True), (key, u)


def _identical_replicates(dev):
    for key in ROWS:
        assert np.all(np.isfinite(dev[key])), key
        assert np.array_equal(dev[key], np.broadcast_to(dev[key][0], dev[key].shape)), key


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("nsamples", pc.REP_COUNTS)
def test_replicate_tiles_match_the_definition(gpu_required, nsamples, bootstrap):
    """One, two and three tiles of 64 replicates in one block, either side of the tile edges; with the bootstrap about a third
    of the replicates draw only the two empty runs and are NaN in all four outputs."""
    case = pc.case(*pc.SMALL, 3, pad=2)
    kw = dict(mode="random", bootstrap=bootstrap)
    timing = {}
    dev = _device(case, nsamples, timing=timing, **kw)
    assert timing["blocks"] == 1 and timing["slabs"] == 1 and timing["columns"] == 13 and timing["elements"] == nsamples * 130
    empty = np.isneginf(dev["logz"])
    assert (0 < empty.sum() < nsamples) if bootstrap else not empty.any()
    for key in ROWS:
        assert dev[key].shape == (nsamples, 3)
        assert np.all(np.isnan(dev[key][empty])) and np.all(np.isfinite(dev[key][~empty])), key
    assert np.all(dev["lpd"][~empty, 1] == pc.CONSTANT) and np.all(dev["var"][~empty, 1] == 0.0)
    pc.check(dev, *case, nsamples, seed=pc.SEED, **kw)


@pytest.mark.parametrize("bootstrap", [False, True])
def test_a_replicate_has_the_same_bits_in_any_tile_and_any_block(gpu_required, bootstrap):
    case = pc.case(*pc.SMALL, 3, pad=2)
    n = case[1].size
    kw = dict(mode="random", bootstrap=bootstrap)
    most = max(pc.REP_COUNTS)
    whole = _device(case, most, **kw)
    one_tile = _device(case, 64, **kw)
    for key in pc.KEYS + ("waic", "logz", "information"):
        assert np.array_equal(whole[key][:64], one_tile[key], equal_nan=True), key
    slab = pointwise.slab_rows()
    timing = {}
    blocks = _device(case, most, timing=timing, **kw,
                     block_bytes=pointwise.table_bytes(n, 3, slab) + 64 * pointwise.replicate_bytes(n, 3, slab))
    assert timing["blocks"] == -(-most // 64) == 3
    pc.same_bits(whole, blocks)


def test_the_same_weights_give_the_same_bits_in_every_slot_of_every_tile(gpu_required):
    """Expected shrinkage without the bootstrap: 130 replicates with the same weights."""
    case = pc.case(*pc.SMALL, 3, pad=2)
    kw = dict(mode="expected", bootstrap=False)
    dev = _device(case, max(pc.REP_COUNTS), **kw)
    _identical_replicates(dev)
    pc.check(dev, *case, max(pc.REP_COUNTS), seed=pc.SEED, **kw)


@pytest.mark.parametrize("bootstrap", [False, True])
def test_blocks_that_straddle_the_replicate_tiles(gpu_required, bootstrap):
    """150 replicates in blocks of 70, 70 and 10: two tiles a block, the second one of 6 replicates, s0 = 70 and 140."""
    case = pc.case(*pc.SMALL, 3, pad=2)
    n, slab = case[1].size, pointwise.slab_rows()
    nsamples, per_block = pc.BLOCK_REPS
    kw = dict(mode="random", bootstrap=bootstrap)
    one = _device(case, nsamples, **kw)
    timing = {}
    blocks = _device(case, nsamples, timing=timing, **kw,
                     block_bytes=pointwise.table_bytes(n, 3, slab) + per_block * pointwise.replicate_bytes(n, 3, slab))
    assert timing["blocks"] == 3 and timing["elements"] == nsamples * n
    pc.same_bits(one, blocks)
    pc.check(blocks, *case, nsamples, seed=pc.SEED, **kw)


@pytest.mark.parametrize("units", pc.WIDE_UNITS)
def test_column_tiles_match_the_definition_and_a_unit_alone(gpu_required, units):
    """61 | 65 and 125 | 129 columns sit either side of the first and the second tile edge, 193 columns open a fourth tile; a
    unit of every tile, the last unit (whose last column is alone in its tile at 16, 32 and 48 units) and the twins."""
    case = pc.case(*pc.SMALL, units)
    constant, (u, v) = pc.layout(units)
    kw = dict(mode="random", bootstrap=False)
    timing = {}
    dev = _device(case, pc.WIDE_REPS, timing=timing, **kw)
    assert timing["columns"] == 4 * units + 1 and timing["blocks"] == 1 and timing["unit_blocks"] == 1
    pc.check(dev, *case, pc.WIDE_REPS, seed=pc.SEED, **kw)
    for key in ("lpd", "loo", "mean"):
        assert np.all(dev[key][:, constant] == pc.CONSTANT), key
    assert np.all(dev["var"][:, constant] == 0.0)
    for key in ROWS:
        assert np.array_equal(dev[key][:, u], dev[key][:, v]), key
    for w in sorted({7, 23, 40, units - 1} & set(range(units))):
        _same_unit(dev, w, _device(_unit(case, w), pc.WIDE_REPS, **kw))


@pytest.mark.parametrize("units", pc.LIMIT_UNITS)
def test_the_unit_limit_and_one_more(gpu_required, units):
    """4096 units are 16385 columns, 257 column tiles, of one call; 4097 go in two (4096 and 1)."""
    case = pc.case(*pc.SMALL, units)
    constant, (u, v) = pc.layout(units)
    kw = dict(mode="random", bootstrap=False)
    timing = {}
    dev = _device(case, 3, timing=timing, **kw)
    assert timing["unit_blocks"] == units - 4095 and timing["columns"] == 4 * units + timing["unit_blocks"]
    pc.check(dev, *case, 3, seed=pc.SEED, **kw)
    assert np.all(dev["lpd"][:, constant] == pc.CONSTANT) and np.all(dev["var"][:, constant] == 0.0)
    for key in ROWS:
        assert np.array_equal(dev[key][:, u], dev[key][:, v]), key
    for w in (0, 2731, units - 1):
        _same_unit(dev, w, _device(_unit(case, w), 3, **kw))


@pytest.mark.parametrize("mode", ["expected", "random"])
@pytest.mark.parametrize("n", pc.ROW_EDGES)
def test_row_counts_at_the_kstep_the_lookahead_and_the_chunk_edges(gpu_required, n, mode):
    case = pc.case(n, max(1, n // 16), 3)
    kw = dict(mode=mode, bootstrap=False)
    timing = {}
    dev = _device(case, pc.WIDE_REPS, timing=timing, **kw)
    assert timing["rows"] == n and timing["slabs"] == 1
    pc.check(dev, *case, pc.WIDE_REPS, seed=pc.SEED, **kw)
    if mode == "expected":
        _identical_replicates(dev)


@pytest.mark.parametrize("mode", ["expected", "random"])
@pytest.mark.parametrize("edge", range(5))
def test_row_counts_at_the_slab_edges(gpu_required, edge, mode):
    slab = pointwise.slab_rows()
    n = pc.slab_edges(slab)[edge]
    case = pc.case(n, n // 80, 3)
    kw = dict(mode=mode, bootstrap=False)
    timing = {}
    dev = _device(case, pc.WIDE_REPS, timing=timing, **kw)
    assert timing["rows"] == n and timing["slabs"] == (1, 1, 2, 2, 3)[edge]
    pc.check(dev, *case, pc.WIDE_REPS, seed=pc.SEED, **kw)
    if mode == "expected":
        _identical_replicates(dev)
