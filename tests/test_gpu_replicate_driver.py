"""The driver that the four merged-run entry points share (rvll_merge_setup.hip: Replicates), through them: rvll_merge_replicates,
rvll_posterior_replicates, rvll_fip_replicates and rvll_marginal_replicates on one input of 3 runs (one of them empty) and 700
rows, with ties in log-L and off-contour rows, 7 replicates, both shrinkage modes with and without the run bootstrap.  Each
entry point is called with block bounds that hold 1, 2 and 7 replicates next to its tables: it must take ceil(7 / s_blk)
blocks, return the same logz and information as every other entry point in every splitting (a wrong first replicate of the
second block would show here), and return its own outputs bit for bit whatever the splitting.  Then every entry point is called
21 times with the bound of exactly one replicate, and the device's free memory must not drift: everything the driver's
allocator hands out, and everything freed before the first block, goes back."""
import ctypes as C

import numpy as np
import pytest

from evidence_amd import fip, marginals, merge, posterior
from test_fip_merged_host import _grid, _periods
from test_merge_host import _arrays, _synthetic
from test_posterior_host import _columns

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

S = 7
NPLANETS = 2
_INPUT = {}


def _input():
    """Built once, shared, never changed."""
    if not _INPUT:
        rng = np.random.default_rng(23)
        empty = (np.zeros(0), np.zeros(0))
        logl, birth, run_start = _arrays([_synthetic(rng, 20, 400, kbatch=4, tie_grid=0.5, off=3), empty,
                                          _synthetic(rng, 10, 270, tie_grid=0.5, off=2)])
        n = logl.size
        assert n == 700 and list(np.diff(run_start)) == [420, 0, 280]
        assert np.unique(logl).size < n and (logl <= birth).sum() >= 4           # ties, off-contour rows
        values = _columns(n, 3)
        _, nua, nub = _grid()
        axes = [(0, np.linspace(-9.0, 9.0, 41)), (1, np.round(np.arange(0.0, 4.01, 0.1), 1)), (0, np.linspace(-8.0, 8.0, 17)),
                (2, 4.23 + np.linspace(-4e-5, 4e-5, 9))]
        panels = [0, 1, (2, 3)]
        _INPUT.update(logl=logl, birth=birth, run_start=run_start, values=values, periods=_periods(n, NPLANETS, 12), nua=nua,
                      nub=nub, axes=axes, panels=panels, nbins=40 + 40 + 16 * 8)
        for v in _INPUT.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _INPUT


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _entries():
    """Per entry point: (the call: (per, kw) -> (dict of outputs, blocks), the bytes of its tables, the bytes of one replicate,
    the largest single device buffer of a call whose block holds one replicate)."""
    a = _input()
    n, rows = a["logl"].size, (a["logl"], a["birth"], a["run_start"])
    ncols, nfreq, naxes, npanels, nbins = a["values"].shape[1], a["nua"].size, len(a["axes"]), len(a["panels"]), a["nbins"]

    def call_merge(block_bytes, kw):
        t = {}
        logz, info, logwt = merge.replicates_arrays(*rows, S, return_logwt=True, device=0, block_bytes=block_bytes, timing=t, **kw)
        return dict(logz=logz, information=info, logwt=logwt), t["launches"] - 4

    def call_posterior(block_bytes, kw):
        t = {}
        out = posterior.summarize_arrays(a["values"], *rows, nsamples=S, device=0, block_bytes=block_bytes, timing=t, **kw)
        return out, t["blocks"]

    def call_fip(block_bytes, kw):
        t = {}
        out = fip.merged_tip_arrays(a["periods"], *rows, a["nua"], a["nub"], nsamples=S, device=0, block_bytes=block_bytes,
                                    timing=t, **kw)
        return out, t["blocks"]

    def call_marginal(block_bytes, kw):
        t = {}
        out = marginals.marginals_arrays(a["values"], *rows, a["axes"], a["panels"], nsamples=S, device=0, return_replicates=True,
                                         block_bytes=block_bytes, timing=t, **kw)
        return out, t["blocks"]

    # the largest buffers: the merge's tables are 8 bytes a row (the event stream: 4 bytes for each of 2 N entries); the input's
    # copy is 8 N C (8 N np); the marginal's Welford state is 5 doubles a bin
    return {
        "merge": (call_merge, 0, 8 * n, 8 * n),
        "posterior": (call_posterior, posterior.table_bytes(n, ncols), 8 * n, max(8 * n * ncols, 8 * S * ncols * 3)),
        "fip": (call_fip, fip.merged_table_bytes(n, NPLANETS, nfreq), 8 * n + 16 * nfreq, max(8 * n * NPLANETS, 8 * nfreq, 8 * S)),
        "marginal": (call_marginal, marginals.table_bytes(n, naxes), marginals.replicate_bytes(n, nbins, npanels),
                     max(8 * n * ncols, 40 * nbins, 2 * n * naxes, 8 * (nbins + npanels))),
    }


@pytest.mark.parametrize("bootstrap", [False, True])
@pytest.mark.parametrize("mode", ["random", "expected"])
def test_every_entry_point_gives_the_same_bits_in_blocks_of_one_two_and_all(gpu_required, mode, bootstrap):
    kw = dict(seed=2 ** 64 - 5, mode=mode, bootstrap=bootstrap)
    a = _input()
    logz, info = merge.replicates_arrays(a["logl"], a["birth"], a["run_start"], S, device=0, **kw)   # no weights: one block
    assert np.all(np.isfinite(logz)) or bootstrap
    for name, (call, tables, per_rep, _) in _entries().items():
        whole = None
        for per_block in (S, 2, 1):
            out, blocks = call(tables + per_block * per_rep, kw)
            print(name, "replicates a block", per_block, "blocks", blocks)
            assert blocks == -(-S // per_block), (name, per_block, blocks)
            assert _same(out["logz"], logz) and _same(out["information"], info), (name, per_block)
            if whole is None:
                whole = out
                assert len(out) > 2                                              # logz, information and its own outputs
            for key in whole:
                assert _same(out[key], whole[key]), (name, per_block, key)


def _free_bytes():
    """hipMemGetInfo of device 0 from the HIP runtime that librvll.so itself is bound to — what torch.cuda.mem_get_info() wraps.
    torch imported into this process after the library's first HIP call loads its own bundled copy of the runtime beside it
    (DESIGN §6), and that second copy finds no device."""
    hip = C.CDLL("libamdhip64.so.7")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_device_memory_of_a_call_goes_back(gpu_required):
    kw = dict(seed=9, mode="random", bootstrap=True)
    for name, (call, tables, per_rep, granule) in _entries().items():
        _, blocks = call(tables + per_rep, kw)                                   # the tables and exactly one replicate
        assert blocks == S
        free_first = _free_bytes()
        for _ in range(20):
            call(tables + per_rep, kw)
        free_last = _free_bytes()
        print(name, "free after the first call", free_first, "after 20 more", free_last, "granule", granule)
        assert abs(free_last - free_first) <= granule, (name, free_first - free_last, granule)
