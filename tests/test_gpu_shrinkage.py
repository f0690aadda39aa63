"""Simulated shrinkage on the device (rvll_shrinkage_replicates, shrinkage.replicates(device=0)) against the numpy definition
of evidence_amd/shrinkage.py: ragged runs (n_dead 0 to far above one workgroup's tile, every schedule shape, -1e30 log-L rows,
odd S), the weights, bit-identical results alone and inside a batch and from call to call, a resident 51 Peg ensemble end to
end, and the refusals."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, _abi, run_nested_ensemble, shrinkage
from evidence_amd.callbacks import wrapped_params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

# (n_dead, nlive, kbatch, m): no deaths; fewer deaths than lanes; one death per iteration; a tile and a bit; far above a tile;
# a budget-cut run_nested (m = nlive - 1)
RUNS = [(0, 10, 2, 5), (30, 8, 3, 8), (600, 100, 1, 100), (1100, 400, 100, 400), (12000, 1000, 250, 1000), (512, 64, 1, 63),
        (255, 300, 5, 300)]


def _ragged(runs, seed=0):
    rng = np.random.default_rng(seed)
    logl, meta = [], []
    for i, (n_dead, nlive, kbatch, m) in enumerate(runs):
        dead = np.sort(rng.normal(0, 20, n_dead)) if n_dead else np.zeros(0)
        if n_dead > 4 and i % 2:
            dead[:3] = -1e30                              # the prior's dead zone: rows that carry no weight
        live = (dead[-1] if n_dead else 0.0) + rng.exponential(1.0, m)
        logl.append(np.concatenate([dead, live]))
        meta.append((n_dead, nlive, kbatch))
    run_start = np.concatenate([[0], np.cumsum([len(x) for x in logl])])
    return np.concatenate(logl), run_start, *[list(v) for v in zip(*meta)]


def _close_w(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape
        near = w > -1e4
        assert np.all(np.abs(g[near] - w[near]) <= 1e-9), float(np.max(np.abs(g[near] - w[near])))
        assert np.all(np.abs(g[~near] - w[~near]) <= 1e-12 * np.abs(w[~near]))


@pytest.mark.parametrize("nsamples", [1, 7, 64])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_device_matches_the_definition(gpu_required, nsamples, mode):
    logl, run_start, n_dead, nlive, kbatch = _ragged(RUNS)
    seeds = [11, 2 ** 64 - 1, 0, 5, 123456789, 77, 3]
    want = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode, return_logwt=True)
    timing = {}
    got = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode, return_logwt=True,
                                      device=0, timing=timing)
    assert np.all(np.abs(got[0] - want[0]) <= 1e-9), float(np.max(np.abs(got[0] - want[0])))
    assert np.all(np.abs(got[1] - want[1]) <= 1e-9), float(np.max(np.abs(got[1] - want[1])))
    assert np.all(got[1][0] == 0.0)
    _close_w(got[2], want[2])
    assert timing["elements"] == logl.size * nsamples and timing["launches"] == 1 and timing["kernel_ms"] > 0
    # without the weights: the same bits
    plain = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, nsamples, mode, device=0)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])


def test_weights_in_several_blocks(gpu_required):
    logl, run_start, n_dead, nlive, kbatch = _ragged(RUNS, seed=1)
    seeds = list(range(len(RUNS)))
    one = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, 9, return_logwt=True, device=0)
    timing = {}
    # 2 replicates of every run per block: 5 launches, the last one short
    few = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, 9, return_logwt=True, device=0,
                                      block_bytes=2 * 8 * logl.size + 8, timing=timing)
    assert timing["launches"] == 5
    assert np.array_equal(one[0], few[0]) and np.array_equal(one[1], few[1])
    assert all(np.array_equal(a, b) for a, b in zip(one[2], few[2]))


def test_a_run_alone_is_the_run_in_a_batch(gpu_required):
    logl, run_start, n_dead, nlive, kbatch = _ragged(RUNS, seed=2)
    seeds = [40 + r for r in range(len(RUNS))]
    batch = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, 33, return_logwt=True, device=0)
    again = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, seeds, 33, return_logwt=True, device=0)
    assert np.array_equal(batch[0], again[0]) and np.array_equal(batch[1], again[1])
    assert all(np.array_equal(a, b) for a, b in zip(batch[2], again[2]))
    for r in (1, 4, 6):
        a, b = run_start[r], run_start[r + 1]
        alone = shrinkage.replicates_arrays(logl[a:b], [0, b - a], n_dead[r:r + 1], nlive[r:r + 1], kbatch[r:r + 1],
                                            seeds[r:r + 1], 33, return_logwt=True, device=0)
        assert np.array_equal(alone[0][0], batch[0][r]) and np.array_equal(alone[1][0], batch[1][r])
        assert np.array_equal(alone[2][0], batch[2][r])


def _51peg():
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def test_51peg_resident_ensemble_end_to_end(gpu_required):
    with _51peg() as m:
        got = run_nested_ensemble(None, None, m.ndim, list(range(1, 9)), live=m, nlive=400, dlogz=0.5,
                                  wrapped=wrapped_params(m.parnames), max_calls=8_000_000)
    assert all((g.nlive, g.kbatch) == (400, 100) for g in got)
    dev = shrinkage.replicates(got, nsamples=101, seed=5, device=0, return_logwt=True)
    ref = shrinkage.replicates(got, nsamples=101, seed=5, return_logwt=True)
    assert np.all(np.abs(dev[0] - ref[0]) <= 1e-9) and np.all(np.abs(dev[1] - ref[1]) <= 1e-9)
    _close_w(dev[2], ref[2])
    exp_z, exp_h = shrinkage.replicates(got, nsamples=3, device=0, mode="expected")
    assert np.all(np.abs(exp_z - np.array([g.logz for g in got])[:, None]) <= 1e-9)
    # (H sums w logl over log-L values far from 0: its round-off is ~1e-10 relative)
    assert np.all(np.abs(exp_h - np.array([g.information for g in got])[:, None]) <= 1e-8)
    err = shrinkage.logz_error(got, nsamples=500, device=0)
    assert np.all(err > 0) and np.all(np.abs(np.log(err / np.array([g.logzerr for g in got]))) < np.log(3))


def test_oversize_weights_are_refused_with_nomem(gpu_required):
    logl, run_start, n_dead, nlive, kbatch = _ragged(RUNS[:3])
    with pytest.raises(RvllError) as exc:
        shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, [1, 2, 3], 4, return_logwt=True, device=0,
                                    block_bytes=8 * logl.size - 8)
    assert exc.value.code == _abi.E_NOMEM
    # the same call within the bound works, and the handle-free entry is left usable
    shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, [1, 2, 3], 4, return_logwt=True, device=0,
                                block_bytes=8 * logl.size)


def _raw(logl, run_start, n_dead, nlive, kbatch, nsamples=2, mode=0):
    """rvll_shrinkage_replicates straight from ctypes, past the Python checks; returns the code."""
    lib = _abi.load()
    R = len(run_start) - 1
    logl = np.ascontiguousarray(logl, dtype=np.float64)
    rs, nd = np.ascontiguousarray(run_start, dtype=np.int64), np.ascontiguousarray(n_dead, dtype=np.int64)
    nl, kb = np.ascontiguousarray(nlive, dtype=np.int32), np.ascontiguousarray(kbatch, dtype=np.int32)
    seeds = np.zeros(max(R, 1), dtype=np.uint64)
    out = np.zeros(max(R, 1) * max(nsamples, 1) * 2)
    p64 = C.POINTER(C.c_int64)
    return lib.rvll_shrinkage_replicates(0, _abi.as_dp(logl), logl.size, rs.ctypes.data_as(p64), R, nd.ctypes.data_as(p64),
                                         _abi.as_ip(nl), _abi.as_ip(kb), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         nsamples, mode, _abi.as_dp(out), _abi.as_dp(out[out.size // 2:]), None, 0, None)


@pytest.mark.parametrize("args", [
    dict(n_dead=[3]),                                   # not a multiple of kbatch
    dict(kbatch=[5]),                                   # kbatch >= nlive
    dict(kbatch=[0]),
    dict(n_dead=[-2]),
    dict(n_dead=[10]),                                  # m = 0
    dict(run_start=[0, 9]),                             # does not add up to the rows
    dict(nsamples=0),
    dict(mode=2),
])
def test_malformed_inputs_are_refused_by_the_entry(gpu_required, args):
    kw = dict(logl=np.zeros(10), run_start=[0, 10], n_dead=[4], nlive=[5], kbatch=[2])
    kw.update(args)
    assert _raw(**kw) == _abi.E_INVALID
    assert _raw(np.zeros(10), [0, 10], [4], [5], [2]) == _abi.OK
