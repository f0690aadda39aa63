"""The device region sampler (rvll_region_draw_runs, GpuRVModel.region_draw_runs) against its numpy definition
(evidence_amd/region.py) on the 51 Peg data: candidates to 1e-13 (Box-Muller and pow differ in their last bits between libm and
the device), every decision exactly from the device's own candidates, independence of the batching, and nested sampling with
proposal="region" through the device entry."""
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, clustering, nested, region, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.config import read_config
from evidence_amd.nested import run_nested_slice

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

CFG = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
KDRAW = 8
SMALL_BLOCK, LARGE_BLOCK = 8, 600            # several rounds of one partly filled workgroup; three workgroups a run, the last ragged
CAP = 4800                                   # candidates per run: a multiple of both blocks


def _model(nplanets=1):
    _rundict, datadict, priordict, fixed = read_config(CFG, nplanets=nplanets)
    return GpuRVModel(fixed, datadict, list(priordict), priordict=priordict)


def _one_wrapped(m):
    wr = np.zeros(m.ndim, dtype=bool)
    wr[np.flatnonzero(wrapped_params(m.parnames))[0]] = True
    return wr


def _runs(m, sizes, wr, seed):
    """One run per entry of sizes: survivors from a tight cloud around the best of a prior sample (so that no ball meets its
    own image in the wrapped dimension), above the cloud's 30 % log-L quantile, in rank order, with their MLFriends region."""
    rng = np.random.default_rng(seed)
    cube = rng.random((4096, m.ndim))
    centre = cube[np.argmax(m.prior_loglike_batch(cube)[1])]
    runs = []
    for r, n in enumerate(sizes):
        cloud = centre + 0.03 * rng.standard_normal((2 * n + 64, m.ndim))
        cloud[:, wr] %= 1.0
        cloud = np.clip(cloud, 0.0, np.nextafter(1.0, 0.0))
        logl = m.prior_loglike_batch(cloud)[1]
        lstar = float(np.quantile(logl, 0.3))
        u = cloud[logl > lstar][:n]
        assert len(u) == n
        u = u[np.argsort(logl[logl > lstar][:n], kind="stable")]
        scale = nested._cluster_scale(u)
        radius2 = clustering.cluster_one(u, scale, wr, 30, 40 + r)[2]
        assert not region.blocked(scale, radius2, wr)
        runs.append((u, scale, radius2, lstar, 900 + 13 * r + seed))
    return runs


def _args(runs):
    return (np.concatenate([r[0] for r in runs]), np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])]).astype(np.int64),
            np.stack([r[1] for r in runs]), np.array([r[2] for r in runs]), np.array([r[3] for r in runs]), [r[4] for r in runs])


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[:5], b[:5]))


def _fragile(t, u, scale, radius2, lstar, seed, wr):
    """The definition's candidates within 1e-12 relative of a boundary: a cube wall, d2 = radius2 for some survivor, U n = 1,
    log-L = lstar."""
    tol = 1e-12
    x = t["cube"]
    wall = np.any((np.abs(x[:, ~wr]) <= tol) | (np.abs(x[:, ~wr] - 1.0) <= tol), axis=1)
    d2 = clustering.pair_d2(x, u, scale, wr)
    edge = np.any(np.abs(d2 - radius2) <= tol * radius2, axis=1)
    un = region.uniform_at(np.uint64(seed), region.counters(t["c"], region.THIN)) * t["n"]
    thin = np.abs(un - 1.0) <= tol
    with np.errstate(invalid="ignore"):
        contour = np.abs(t["logl"] - lstar) <= tol * abs(lstar)
    return wall | edge | thin | contour


def _check_decisions(m, t, out, u, scale, radius2, lstar, seed, wr, kdraw):
    """Everything that follows from the device's own candidates, exactly."""
    cube, theta, logl, nfound, ncalls = out
    x = t["cube"]
    outside = np.any(~((x[:, ~wr] >= 0.0) & (x[:, ~wr] < 1.0)), axis=1)
    assert np.array_equal((t["flags"] & region.OUTSIDE) != 0, outside)
    assert np.all((x[:, wr] >= 0.0) & (x[:, wr] < 1.0))
    n = region.neighbours(x, u, scale, radius2, wr)
    assert np.array_equal(t["n"][~outside], n[~outside]) and np.all(t["n"][outside] == 0)
    assert np.array_equal((t["flags"] & region.LOST) != 0, ~outside & (n == 0))
    kept = ~outside & region.thin_keep(seed, t["c"], t["n"])
    assert np.array_equal((t["flags"] & region.KEPT) != 0, kept)
    ref_theta, ref_logl = m.prior_loglike_batch(x[kept])
    assert t["logl"][kept].tobytes() == ref_logl.tobytes() and np.all(np.isnan(t["logl"][~kept]))
    accepted = kept & (t["logl"] > lstar)
    assert np.array_equal((t["flags"] & region.ACCEPTED) != 0, accepted)
    take, calls = region.select(kept, accepted, kdraw)           # (one block holding every candidate: the definition's rule)
    assert nfound == len(take) and ncalls == calls
    assert cube[:nfound].tobytes() == x[take].tobytes() and logl[:nfound].tobytes() == t["logl"][take].tobytes()
    kept_rows = np.cumsum(kept) - 1
    assert theta[:nfound].tobytes() == ref_theta[kept_rows[take]].tobytes()
    assert np.all(np.isnan(cube[nfound:])) and np.all(np.isnan(logl[nfound:]))


def test_candidates_and_decisions_match_the_definition(gpu_required):
    """R = 3 runs of 40, 64 (one full wave pass over the survivors) and 200 (ragged against wave and workgroup) survivors, one
    wrapped dimension, kdraw = 8, a block of 8 candidates: at least three rounds."""
    with _model() as m:
        wr = _one_wrapped(m)
        runs = _runs(m, [40, 64, 200], wr, 1)
        surv, run_start, scale, radius2, lstar, seeds = _args(runs)

        def evaluate(c):
            return m.prior_loglike_batch(c)
        ref = region.draw_runs(surv, run_start, scale, radius2, lstar, seeds, KDRAW, evaluate, wrapped=wr, max_candidates=CAP,
                               trace=True, block=SMALL_BLOCK)
        # the definition alone: fragile candidates stay below 1 %
        nfrag = ncand = 0
        frag = []
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            frag.append(_fragile(ref[5][r], u, sc, r2, ls, sd, wr))
            nfrag += int(np.count_nonzero(frag[-1])); ncand += len(frag[-1])
        print(f"{nfrag} fragile candidates of {ncand}")
        assert ncand > 0 and nfrag < 0.01 * ncand
        got = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, KDRAW, wrapped=wr, max_candidates=CAP, trace=True,
                                 block=SMALL_BLOCK, return_rounds=True)
        print("rounds", got[6], "nfound", got[3], "ncalls", got[4], "definition", ref[3], ref[4])
        assert got[6] >= 3
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            t, tr = got[5][r], ref[5][r]
            assert len(t["c"]) > 0 and len(t["c"]) % SMALL_BLOCK == 0
            k = min(len(t["c"]), len(tr["c"]))
            assert k > 0 and np.array_equal(t["c"][:k], tr["c"][:k])
            ok = ~frag[r][:k]
            err = t["cube"][:k][ok] - tr["cube"][:k][ok]
            err[:, wr] -= np.rint(err[:, wr])                        # (a fold next to 0 may land on either side of it)
            err = np.abs(err)
            print(f"run {r}: {k} candidates, max |device - definition| = {err.max():.3e}")
            assert err.max() <= 1e-13
            _check_decisions(m, t, [x[r] for x in got[:5]], u, sc, r2, ls, sd, wr, KDRAW)
            if not frag[r].any() and len(t["c"]) == len(tr["c"]):     # no candidate near a boundary: the same decisions throughout
                assert np.array_equal(t["flags"], tr["flags"]) and np.array_equal(t["n"], tr["n"])
                assert got[3][r] == ref[3][r] and got[4][r] == ref[4][r]


def test_results_do_not_depend_on_the_batching(gpu_required):
    with _model() as m:
        wr = _one_wrapped(m)
        tile = m.region_tile_rows()
        assert tile == 5120 // m.ndim
        runs = _runs(m, [40, 64, 200, tile + 1], wr, 2)       # the last: the smallest run the neighbour count has to tile
        surv, run_start, scale, radius2, lstar, seeds = _args(runs)
        kw = dict(wrapped=wr, max_candidates=CAP, trace=True)
        small = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, KDRAW, block=SMALL_BLOCK, **kw)
        large = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, KDRAW, block=LARGE_BLOCK, **kw)
        assert _same(small, large)
        assert np.all(small[3] > 0)
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            for out in (small, large):
                _check_decisions(m, out[5][r], [x[r] for x in out[:5]], u, sc, r2, ls, sd, wr, KDRAW)
            k = len(small[5][r]["c"])                          # the small blocks' candidates are the first of the large block's
            assert k <= len(large[5][r]["c"])
            for key in ("cube", "flags", "n", "logl"):
                assert small[5][r][key].tobytes() == large[5][r][key][:k].tobytes(), (r, key)
        # run 1 alone against run 1 among the others
        rows = slice(run_start[1], run_start[2])
        alone = m.region_draw_runs(surv[rows], [0, 64], scale[1:2], radius2[1:2], lstar[1:2], seeds[1:2], KDRAW, block=LARGE_BLOCK, **kw)
        assert _same(alone, [x[1:2] for x in large[:5]])
        # a partial draw: the cap runs out first
        part = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, 10 ** 4, wrapped=wr, max_candidates=700, trace=True,
                                  block=LARGE_BLOCK)
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            assert len(part[5][r]["c"]) == 700 and part[3][r] < 10 ** 4
            _check_decisions(m, part[5][r], [x[r] for x in part[:5]], u, sc, r2, ls, sd, wr, 10 ** 4)


HIGH_KDRAW = 64
HIGH_CAP = 4800


def _high_wrapped(ndim):
    wr = np.zeros(ndim, dtype=bool)
    wr[ndim - 1] = True                      # bit 32 of the mask at 33 dimensions, bit 63 at 64
    if ndim > 35:
        wr[35] = True                        # a second bit of the high word, not the last (64 dimensions only: 33 has no such)
    return wr


def _high_runs(evaluate, ndim, sizes, wr, seed):
    """_runs for a model of ndim offsets.  The cloud's centre lies at 0.5 +- 0.01, but for coordinates 0 and 1 (not wrapped),
    which lie at 0.02 and 0.985: candidates cross both walls.  The contour of the draw is the midpoint of the two middle log-L
    values among the kept ones of the definition's first 512 candidates (drawn with lstar = +inf, so that none is taken): about
    half of the kept candidates are accepted at any ndim, and the contour lies on none of them."""
    rng = np.random.default_rng(seed)
    centre = 0.5 + rng.uniform(-0.01, 0.01, ndim)
    centre[0], centre[1] = 0.02, 0.985
    runs = []
    for r, n in enumerate(sizes):
        cloud = centre + 0.03 * rng.standard_normal((2 * n + 64, ndim))
        cloud[:, wr] %= 1.0
        cloud = np.clip(cloud, 0.0, np.nextafter(1.0, 0.0))
        logl = evaluate(cloud)[1]
        floor = float(np.quantile(logl, 0.3))
        u = cloud[logl > floor][:n]
        assert len(u) == n
        u = u[np.argsort(logl[logl > floor][:n], kind="stable")]
        scale = nested._cluster_scale(u)
        radius2 = clustering.cluster_one(u, scale, wr, 30, 40 + r)[2]
        assert not region.blocked(scale, radius2, wr)
        sd = 900 + 13 * r + seed
        pre = region.draw_runs(u, [0, n], scale[None], [radius2], [np.inf], [sd], HIGH_KDRAW, evaluate, wrapped=wr,
                               max_candidates=512, trace=True, block=512)[5][0]
        kept = np.sort(pre["logl"][(pre["flags"] & region.KEPT) != 0])
        assert kept.size >= 2 and kept[kept.size // 2 - 1] < kept[kept.size // 2]
        lstar = 0.5 * (kept[kept.size // 2 - 1] + kept[kept.size // 2])
        runs.append((u, scale, radius2, float(lstar), sd))
    return runs


@pytest.mark.parametrize("ndim", [8, 9, 16, 17, 32, 33, 64])
def test_every_dimension_template_matches_the_definition(gpu_required, ndim):
    """Both sides of every edge of the propose kernel's register templates (8, 16, 32 and 64 coordinates: 8 | 9, 16 | 17,
    32 | 33, and 64 itself), on a model of ndim instrument offsets: the last dimension wrapped, and dimension 35 too where there
    is one (bits of the mask's high word); runs of 40 survivors and of one more than the LDS tile holds.  With the definition
    alone: candidates leave the cube, every run gets its 64 draws, under 1 % of the candidates are fragile, and up to 17
    dimensions some candidate lies in more than one ball (beyond, the balls of so thin a cloud hardly overlap)."""
    from test_gpu_clustering import _offsets_model
    with _offsets_model(ndim) as m:
        tile = m.region_tile_rows()
        assert tile == 5120 // ndim
        wr = _high_wrapped(ndim)
        runs = _high_runs(m.prior_loglike_batch, ndim, [40, tile + 1], wr, ndim)
        surv, run_start, scale, radius2, lstar, seeds = _args(runs)
        kw = dict(wrapped=wr, max_candidates=HIGH_CAP, trace=True)
        ref = region.draw_runs(surv, run_start, scale, radius2, lstar, seeds, HIGH_KDRAW, m.prior_loglike_batch, block=SMALL_BLOCK,
                               **kw)
        frag = [_fragile(ref[5][r], u, sc, r2, ls, sd, wr) for r, (u, sc, r2, ls, sd) in enumerate(runs)]
        flags = np.concatenate([t["flags"] for t in ref[5]])
        ncand, nfrag = flags.size, int(sum(np.count_nonzero(f) for f in frag))
        counts = {name: int(np.count_nonzero(flags & bit)) for name, bit in (("outside", region.OUTSIDE), ("lost", region.LOST),
                                                                              ("kept", region.KEPT), ("accepted", region.ACCEPTED))}
        nmax = max(int(t["n"].max()) for t in ref[5])
        print(f"D = {ndim}: {ncand} candidates, {counts}, largest n {nmax}, {nfrag} fragile, nfound {ref[3]}, ncalls {ref[4]}")
        assert counts["outside"] > 0 and counts["kept"] > 0 and np.all(ref[3] == HIGH_KDRAW)
        assert nfrag < 0.01 * ncand
        assert ndim > 17 or nmax > 1
        small = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, HIGH_KDRAW, block=SMALL_BLOCK, **kw)
        large = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, HIGH_KDRAW, block=LARGE_BLOCK, **kw)
        assert _same(small, large)
        worst = 0.0
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            t, tr = small[5][r], ref[5][r]
            k = min(len(t["c"]), len(tr["c"]))
            assert k > 0 and len(t["c"]) % SMALL_BLOCK == 0 and np.array_equal(t["c"][:k], tr["c"][:k])
            ok = ~frag[r][:k]
            err = t["cube"][:k][ok] - tr["cube"][:k][ok]
            err[:, wr] -= np.rint(err[:, wr])
            worst = max(worst, float(np.abs(err).max()))
            for out in (small, large):
                _check_decisions(m, out[5][r], [x[r] for x in out[:5]], u, sc, r2, ls, sd, wr, HIGH_KDRAW)
            if not frag[r].any() and len(t["c"]) == len(tr["c"]):
                assert np.array_equal(t["flags"], tr["flags"]) and np.array_equal(t["n"], tr["n"])
                assert small[3][r] == ref[3][r] and small[4][r] == ref[4][r]
            kk = len(t["c"])
            assert kk <= len(large[5][r]["c"])
            for key in ("cube", "flags", "n", "logl"):
                assert t[key].tobytes() == large[5][r][key][:kk].tobytes(), (r, key)
        print(f"D = {ndim}: max |device - definition| = {worst:.3e}")
        assert worst <= 1e-13


def test_the_offsets_carry_and_every_select_pass(gpu_required):
    """65 runs of 40 survivors with a block of 1024 candidates: 260 workgroups, which the offsets kernel scans 256 at a time,
    so the four workgroups of run 64 start at the carry of the first step; and select takes four passes of 256 over a block
    (sixteen over the default block of 4096), its counts of accepted and kept candidates carried from pass to pass.  The runs
    that evaluate more than 256 candidates with the small block take draws past select's first pass."""
    with _model() as m:
        wr = _one_wrapped(m)
        runs = _runs(m, [40] * 65, wr, 4)
        surv, run_start, scale, radius2, lstar, seeds = _args(runs)
        kw = dict(wrapped=wr, max_candidates=8192, trace=True)
        small = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, HIGH_KDRAW, block=SMALL_BLOCK, **kw)
        wide = m.region_draw_runs(surv, run_start, scale, radius2, lstar, seeds, HIGH_KDRAW, block=1024, return_rounds=True, **kw)
        evaluated = np.array([len(t["c"]) for t in small[5]])
        print("candidates a run evaluated with the small block: min", evaluated.min(), "median", int(np.median(evaluated)), "max",
              evaluated.max(), " nfound", small[3].min(), small[3].max(), " rounds of the block of 1024:", wide[6])
        assert np.all(small[3] == HIGH_KDRAW) and np.count_nonzero(evaluated > 256) >= 33 and evaluated[64] > 256
        assert _same(small, wide)
        for r, (u, sc, r2, ls, sd) in enumerate(runs):
            assert len(wide[5][r]["c"]) % 1024 == 0 and len(wide[5][r]["c"]) >= evaluated[r]
            _check_decisions(m, wide[5][r], [x[r] for x in wide[:5]], u, sc, r2, ls, sd, wr, HIGH_KDRAW)
        rows = slice(run_start[64], run_start[65])
        alone = m.region_draw_runs(surv[rows], [0, 40], scale[64:65], radius2[64:65], lstar[64:65], seeds[64:65], HIGH_KDRAW,
                                   block=1024, **kw)
        assert _same(alone, [x[64:65] for x in wide[:5]])
        four = slice(0, run_start[4])
        default = m.region_draw_runs(surv[four], run_start[:5], scale[:4], radius2[:4], lstar[:4], seeds[:4], HIGH_KDRAW, **kw)
        assert all(len(t["c"]) == 4096 for t in default[5])
        assert _same(default, [x[:4] for x in small[:5]])
        for r, (u, sc, r2, ls, sd) in enumerate(runs[:4]):
            _check_decisions(m, default[5][r], [x[r] for x in default[:5]], u, sc, r2, ls, sd, wr, HIGH_KDRAW)


def test_blocked_and_empty_runs_and_argument_errors(gpu_required):
    from evidence_amd import _abi
    with _model() as m:
        wr = _one_wrapped(m)
        (u, sc, r2, ls, sd), = _runs(m, [40], wr, 3)
        k = int(np.flatnonzero(wr)[0])
        wide = float((0.5 * sc[k]) ** 2) * 1.0001                      # the ball meets its own image in the wrapped dimension
        assert region.blocked(sc, wide, wr)
        out = m.region_draw_runs(np.concatenate([u, u]), [0, 40, 40, 80], np.stack([sc, sc, sc]), [wide, r2, r2], [ls, ls, ls],
                                 [sd, sd, sd], KDRAW, wrapped=wr, max_candidates=CAP)
        assert out[3][0] == 0 and out[4][0] == 0 and out[3][1] == 0 and out[4][1] == 0 and out[3][2] > 0
        for bad in (dict(scale=-sc[None]), dict(radius2=[np.inf])):
            kw = dict(survivors=u, run_start=[0, 40], scale=sc[None], radius2=[r2], lstar=[ls], seeds=[sd], kdraw=2)
            kw.update(bad)
            with pytest.raises(ValueError):
                m.region_draw_runs(**kw)
        import ctypes as C
        rs = np.array([0, 50, 40], dtype=np.int64)
        found, calls = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
        o = np.zeros((2, 2, m.ndim))
        args = [m._h, _abi.as_dp(u), rs.ctypes.data_as(C.POINTER(C.c_int64)), 2, _abi.as_dp(np.stack([sc, sc])),
                _abi.as_dp(np.array([r2, r2])), _abi.as_dp(np.array([ls, ls])), np.array([1, 2], dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)),
                None, 2, 0, 100, 64, _abi.as_dp(o), _abi.as_dp(o.copy()), _abi.as_dp(np.zeros((2, 2))), _abi.as_ip(found),
                calls.ctypes.data_as(C.POINTER(C.c_int64)), 0, None, None, None, None, None, None]
        assert m._lib.rvll_region_draw_runs(*args) == _abi.E_INVALID          # run_start decreases
        args[2] = np.array([0, 20, 40], dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
        args[16] = None
        assert m._lib.rvll_region_draw_runs(*args) == _abi.E_INVALID          # a missing pointer


def test_51peg_region_ensemble_is_its_standalone_runs(gpu_required):
    """51 Peg without a planet (offset and jitter), nlive = 50, two seeds: births are the contours the points were drawn above,
    ncall is the sum of the recorded calls, and every run of the ensemble is the one-seed run bit for bit."""
    with _model(0) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        kw = dict(nlive=50, max_iter=480, dlogz=1e-9, proposal="region", region_runs=m.region_draw_runs, wrapped=wrapped_params(m.parnames))
        ens = run_nested_ensemble(prior, loglike, m.ndim, seeds=[1, 2], **kw)
        alone = [run_nested_slice(prior, loglike, m.ndim, seed=s, **kw) for s in (1, 2)]
    for e, a in zip(ens, alone):
        assert e.niter == a.niter == 480 and e.ncall == a.ncall and e.logz == a.logz and e.logzerr == a.logzerr
        assert np.array_equal(e.samples, a.samples) and np.array_equal(e.logl, a.logl) and np.array_equal(e.logwt, a.logwt)
        assert np.array_equal(e.logl_birth, a.logl_birth) and np.array_equal(e.region_calls, a.region_calls)
        assert e.region_fallbacks == a.region_fallbacks
        print("fallbacks", e.region_fallbacks, "efficiency", np.round(e.region_efficiency, 3))
        assert e.ncall == 50 + int(e.region_calls.sum()) + e.region_fallback_calls
        kb = e.kbatch
        contours = e.logl[:e.niter].reshape(-1, kb)[:, -1]                    # every iteration's lstar: its last death
        born = np.isfinite(e.logl_birth)
        assert np.count_nonzero(born) == e.niter and np.all(np.isin(e.logl_birth[born], contours))
        assert np.all(e.logl[born] > e.logl_birth[born])
        # a point born in iteration i dies in a later one or stays live: its birth is the contour of an earlier iteration
        it_of_row = np.concatenate([np.repeat(np.arange(e.niter // kb), kb), np.full(len(e.logl) - e.niter, e.niter // kb)])
        assert np.all(np.searchsorted(contours, e.logl_birth[born]) < it_of_row[born])
