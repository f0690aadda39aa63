"""The device clustering (rvll_cluster_runs, GpuRVModel.cluster_runs) against its numpy definition
(evidence_amd/clustering.py), bit for bit, and nested sampling with clustering on the GPU: a clustered ensemble is its
standalone clustered runs, a unimodal run is the unclustered run, and the 3-planet model's modes reach the walk as groups."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import GpuRVModel, _abi, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.clustering import cluster_runs as np_cluster_runs
from evidence_amd.nested import run_nested_slice
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def _offsets_model(ndim):
    """A model with ndim free instrument offsets and no planet (the clustering only needs the dimension)."""
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    names = [f"i{k}" for k in range(ndim)]
    table = EpochTable.from_arrays(names, np.arange(1.0, ndim + 1.0), np.zeros(ndim), np.ones(ndim), np.arange(ndim))
    pri = {f"{n}_offset": P.Uniform(-10, 10) for n in names}
    return GpuRVModel({}, table, list(pri), priordict=pri)


def _assert_same(got, ref, what):
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(got[1], ref[1]), (what, got[1], ref[1])
    assert got[2].tobytes() == ref[2].tobytes(), (what, got[2], ref[2])


def _cases(rng, ndim, wrap_dim=0):
    """(name, runs, wrapped): blobs, a blob across the wrap of dimension wrap_dim (the one wrapped dimension), uniform rows, a
    ragged batch with runs of 0, 1 and 2 rows."""
    def blobs(centres, n, sig):
        return np.concatenate([np.clip(rng.normal(c, sig, (n, ndim)), 0.0, np.nextafter(1.0, 0.0)) for c in centres])
    wrap_blob = rng.normal(0.0, 0.02, (120, ndim)) + 0.5
    wrap_blob[:, wrap_dim] = (wrap_blob[:, wrap_dim] - 0.5) % 1.0
    wr = np.zeros(ndim, dtype=bool)
    wr[wrap_dim] = True
    return [("blobs", [blobs([0.2, 0.5, 0.8], 90, 0.02)], None),
            ("wrapped", [wrap_blob], wr),
            ("not wrapped", [wrap_blob], None),
            ("uniform", [rng.random((400, ndim))], None),
            ("ragged", [blobs([0.3, 0.7], 70, 0.03), rng.random((0, ndim)), rng.random((1, ndim)), rng.random((2, ndim)),
                        rng.random((333, ndim)), blobs([0.25, 0.75], 65, 0.01)], wr)]


@pytest.mark.parametrize("ndim", [1, 7, 19, 8, 9, 16, 17, 32, 33, 64])
def test_device_clustering_is_the_numpy_definition(gpu_required, ndim):
    """1, 7 and 19 dimensions with dimension 0 wrapped; then both sides of every edge of the kernels' register templates (rows
    of 8, 16, 32 and 64 doubles: 8 | 9, 16 | 17, 32 | 33, and 64 itself) with the last dimension wrapped: bit 32 of the 64-bit
    mask at 33 dimensions, bit 63 at 64.  The runs of 400 and 333 rows cross the LDS tile (16384 / 8 ndim rows) at every size;
    at 33 and 64 dimensions the tile (62 and 32 rows) is shorter than the 64-row workgroup that loads it."""
    rng = np.random.default_rng(100 + ndim)
    wrap_dim = 0 if ndim in (1, 7, 19) else ndim - 1
    with _offsets_model(ndim) as m:
        for name, runs, wr in _cases(rng, ndim, wrap_dim):
            cube = np.concatenate(runs)
            run_start = np.concatenate([[0], np.cumsum([len(r) for r in runs])]).astype(np.int64)
            scale = rng.uniform(0.5, 4.0, (len(runs), ndim))
            seeds = [int(s) for s in rng.integers(0, 2 ** 63, len(runs))]
            for nboot in (0, 1, 30, 32):
                got = m.cluster_runs(cube, run_start, scale, wr, nboot, seeds)
                _assert_same(got, np_cluster_runs(cube, run_start, scale, wr, nboot, seeds), (ndim, name, nboot))
                if nboot >= 30:                  # (one or no bootstrap gives a small radius: blobs may break up)
                    expect = {"blobs": [3], "wrapped": [1], "not wrapped": [2] if ndim > 1 else None,
                              "uniform": [1], "ragged": [2, 0, 1, 1, 1, 2]}[name]
                    assert expect is None or list(got[1]) == expect, (ndim, name, nboot, got[1])
                if name == "ragged" and nboot == 30:
                    # a batched launch is the runs launched one by one
                    assert list(got[1][1:4]) == [0, 1, 1]
                    for r in range(len(runs)):
                        one = m.cluster_runs(runs[r], [0, len(runs[r])], scale[r:r + 1], wr, nboot, [seeds[r]])
                        rows = slice(run_start[r], run_start[r + 1])
                        _assert_same((got[0][rows], got[1][r:r + 1], got[2][r:r + 1]), one, (ndim, r))


def test_one_run_of_8192_rows(gpu_required):
    rng = np.random.default_rng(7)
    with _offsets_model(7) as m:
        cube = np.concatenate([np.clip(rng.normal(c, 0.05, (4096, 7)), 0.0, np.nextafter(1.0, 0.0)) for c in (0.3, 0.7)])
        cube = cube[rng.permutation(len(cube))]
        scale = np.full((1, 7), 1.0 / 0.05)
        got = m.cluster_runs(cube, [0, 8192], scale, None, 30, [99])
        _assert_same(got, np_cluster_runs(cube, [0, 8192], scale, None, 30, [99]), "8192")
        assert got[1][0] >= 2
        labels, ncl, r2 = m.cluster(cube, scale[0], None, 30, 99)
        assert np.array_equal(labels, got[0]) and ncl == got[1][0] and r2 == got[2][0]


def test_argument_errors_are_invalid(gpu_required):
    rng = np.random.default_rng(8)
    with _offsets_model(3) as m:
        u = rng.random((10, 3))
        bad = [dict(run_start=[0, 10], scale=np.ones((1, 3)), nboot=33, seeds=[0]),
               dict(run_start=[0, 10], scale=np.ones((1, 3)), nboot=-1, seeds=[0]),
               dict(run_start=[0, 6, 4, 10], scale=np.ones((3, 3)), nboot=30, seeds=[0, 1, 2]),
               dict(run_start=[0, 10], scale=np.array([[1.0, 0.0, 1.0]]), nboot=30, seeds=[0]),
               dict(run_start=[0, 10], scale=np.array([[1.0, np.nan, 1.0]]), nboot=30, seeds=[0]),
               dict(run_start=[0, 10], scale=np.array([[1.0, -np.inf, 1.0]]), nboot=30, seeds=[0])]
        for kw in bad:
            with pytest.raises(_abi.RvllError) as e:
                m.cluster_runs(u, kw["run_start"], kw["scale"], None, kw["nboot"], kw["seeds"])
            assert e.value.code == _abi.E_INVALID, kw
        # run_start not starting at 0, and NULL where a buffer is required, through the C-ABI itself
        lib = _abi.load()
        rs = np.array([1, 10], dtype=np.int64)
        out_l, out_n, out_r = np.zeros(10, np.int32), np.zeros(1, np.int32), np.zeros(1)
        seeds = np.zeros(1, np.uint64)
        scale = np.ones(3)
        args = lambda rs_, seeds_: (m._h, _abi.as_dp(u), rs_.ctypes.data_as(C.POINTER(C.c_int64)), 1, _abi.as_dp(scale),   # noqa: E731
                                    None, 30, seeds_, _abi.as_ip(out_l), _abi.as_ip(out_n), _abi.as_dp(out_r))
        assert lib.rvll_cluster_runs(*args(rs, seeds.ctypes.data_as(C.POINTER(C.c_uint64)))) == _abi.E_INVALID
        assert lib.rvll_cluster_runs(*args(np.array([0, 10], np.int64), None)) == _abi.E_INVALID
        assert lib.rvll_cluster_runs(*args(np.array([0, 10], np.int64), seeds.ctypes.data_as(C.POINTER(C.c_uint64)))) == 0


def _same_result(a, b):
    assert a.niter == b.niter and a.ncall == b.ncall and a.logz == b.logz and a.information == b.information
    assert np.array_equal(a.samples, b.samples) and np.array_equal(a.logl, b.logl) and np.array_equal(a.logwt, b.logwt)


def test_51peg_clustered_ensemble_is_its_standalone_clustered_runs(gpu_required):
    from pathlib import Path
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=300, dlogz=0.5, wrapped=wrapped_params(m.parnames), max_calls=3_000_000, clustering=True)
        seeds = [1, 2, 3]
        ens = run_nested_ensemble(prior, loglike, m.ndim, seeds, walker_runs=m.slice_walk_runs, clusterer=m.cluster_runs, **kw)
        for s, got in zip(seeds, ens):
            one = run_nested_slice(prior, loglike, m.ndim, seed=s, walker_runs=m.slice_walk_runs, clusterer=m.cluster_runs, **kw)
            _same_result(got, one)
            assert np.array_equal(got.nclusters, one.nclusters)


def test_unimodal_gaussian_clustered_is_unclustered(gpu_required):
    """The no-planet Gaussian of test_gpu_walk.py: one cluster every iteration, and then the run is the unclustered run."""
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    table = EpochTable.from_arrays(["a", "b"], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], [0, 1])
    pri = {"a_offset": P.Uniform(-10, 10), "b_offset": P.Uniform(-10, 10)}
    with GpuRVModel({}, table, list(pri), priordict=pri) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=1000, dlogz=0.01, nsteps=10, max_calls=20_000_000)
        off = run_nested_slice(prior, loglike, 2, seed=1, walker=m.slice_walk, **kw)
        on = run_nested_slice(prior, loglike, 2, seed=1, clustering=True, walker_runs=m.slice_walk_runs,
                              clusterer=m.cluster_runs, **kw)
    assert np.all(on.nclusters == 1) and len(on.nclusters) > 0
    _same_result(on, off)
    assert abs(on.logz + np.log(400.0)) < 4 * on.logzerr + 0.05


def test_three_planet_modes_reach_the_walk_as_groups(gpu_required):
    w = make_workload(3)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict()) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        calls = []

        def spy(cube, theta, logl, run_start, *rest):
            calls.append(len(run_start) - 1)
            return m.slice_walk_runs(cube, theta, logl, run_start, *rest)

        r = run_nested_slice(prior, loglike, m.ndim, nlive=1500, seed=5, wrapped=wrapped_params(m.parnames), clustering=True,
                             walker_runs=spy, clusterer=m.cluster_runs, max_calls=30_000_000)
    assert int(np.max(r.nclusters)) >= 2, np.unique(r.nclusters)
    assert max(calls) > 1                                       # one run: a call with more walk groups than runs
    assert np.isfinite(r.logz)
