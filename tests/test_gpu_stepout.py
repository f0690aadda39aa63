"""The stepping-out slice proposal on the device (rvll_set_walk_proposal(RVLL_PROPOSAL_STEPOUT)): the walk's
invariants, uniformity, the Gaussian and 51 Peg evidence, and every bit-for-bit equality the chord walk keeps — speculation,
the queue, the slim kernel with its full-solver finish, sharding, run mode, the resident live set and ensemble."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import GpuRVModel, RvllError, run_nested_ensemble
from evidence_amd.callbacks import make_ultranest_callbacks, wrapped_params
from evidence_amd.nested import run_nested_slice
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
SO = dict(proposal="stepout", step_width=1.0)


def _start(m, k, seed, quantile=0.5):
    rng = np.random.default_rng(seed)
    cube = rng.random((k, m.ndim))
    theta, logl = m.prior_loglike_batch(cube)
    lstar = float(np.quantile(logl, quantile))
    keep = logl > lstar
    cube, theta, logl = cube[keep], theta[keep], logl[keep]
    d0 = cube - cube.mean(axis=0)
    chol = np.linalg.cholesky(d0.T @ d0 / (len(cube) - 1) + 1e-14 * np.eye(m.ndim))
    return cube, theta, logl, lstar, chol


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.all(np.asarray(a[3]) == np.asarray(b[3]))


def _model(cfg=3, **kw):
    w = make_workload(cfg)
    return GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=w.priordict(), **kw)


@pytest.mark.parametrize("cfg, k", [(3, 3000), (1, 700)])
def test_stepout_walk_invariants(gpu_required, cfg, k):
    with _model(cfg) as m:
        cube, theta, logl, lstar, chol = _start(m, k, seed=cfg)
        wr = wrapped_params(m.parnames)
        c2, t2, l2, n = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=12, seed=11, **SO)
        th_chk, ll_chk = m.prior_loglike_batch(c2)
        again = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=12, seed=11, **SO)
        other = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=12, seed=12, **SO)
        zero = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=0, seed=11, **SO)
        chord = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=12, seed=11)
    assert (l2 > lstar).all() and ((c2 >= 0) & (c2 < 1)).all()
    assert np.array_equal(th_chk, t2) and np.array_equal(ll_chk, l2)
    assert n >= 12 * len(cube) and np.mean(np.any(c2 != cube, axis=1)) > 0.99
    assert _same((c2, t2, l2, n), again) and not np.array_equal(c2, other[0])
    assert np.array_equal(zero[0], cube) and np.array_equal(zero[2], logl) and zero[3] == 0
    assert not np.array_equal(chord[0], c2)                 # another proposal, other end points


def test_unconstrained_stepout_walk_is_uniform(gpu_required):
    from scipy import stats
    with _model(2) as m:
        k = 8000
        cube = np.full((k, m.ndim), 0.31)
        theta, logl = m.prior_loglike_batch(cube)
        wr = wrapped_params(m.parnames)
        chol = np.diag(np.full(m.ndim, 0.2))
        c, _, _, n = m.slice_walk(cube, theta, logl, -np.inf, chol, wr, nsteps=6 * m.ndim, seed=5, max_rounds=1000, **SO)
    assert n > 6 * m.ndim * k
    for j in range(m.ndim):                                 # walls and circular parameters alike
        assert stats.kstest(c[:, j], "uniform").pvalue > 1e-3, (j, wr[j])


def test_gaussian_evidence_with_the_stepout_walk(gpu_required):
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    table = EpochTable.from_arrays(["a", "b"], [1.0, 2.0], [0.0, 0.0], [1.0, 1.0], [0, 1])
    pri = {"a_offset": P.Uniform(-10, 10), "b_offset": P.Uniform(-10, 10)}
    with GpuRVModel({}, table, list(pri), priordict=pri) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        out = [run_nested_slice(prior, loglike, 2, nlive=1000, dlogz=0.01, seed=s, walker=m.slice_walk, nsteps=10,
                                max_calls=20_000_000, **SO) for s in (1, 2)]
        out += [run_nested_slice(None, None, 2, nlive=1000, dlogz=0.01, seed=s, live=m, nsteps=10, max_calls=20_000_000, **SO)
                for s in (4, 5)]
    for r in out:
        assert abs(r.logz - (-np.log(400.0))) < 4 * r.logzerr + 0.05, (r.logz, r.logzerr)


def test_51peg_evidence_stepout_agrees_with_host_stepout_and_with_the_chord_walk(gpu_required):
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        wrap = wrapped_params(m.parnames)
        kw = dict(nlive=400, dlogz=0.5, wrapped=wrap, max_calls=8_000_000)
        host = run_nested_slice(prior, loglike, m.ndim, seed=1, prior_loglike=m.prior_loglike_batch, nsteps=5 * m.ndim, **kw, **SO)
        dev = run_nested_slice(prior, loglike, m.ndim, seed=2, walker=m.slice_walk, nsteps=5 * m.ndim, **kw, **SO)
        chord = run_nested_slice(prior, loglike, m.ndim, seed=3, walker=m.slice_walk, **kw)
    for other in (host, chord):
        # the sampler scatters by ~1.5 in ln Z from seed to seed on this multimodal posterior (test_gpu_walk.py)
        assert abs(dev.logz - other.logz) < 5 * np.hypot(dev.logzerr, other.logzerr) + 3.0, (dev.logz, other.logz)
    wgt = np.exp(dev.logwt)
    assert abs(np.sum(wgt * dev.samples[:, m.parnames.index("planet1_period")]) - 4.2308) < 0.01


def test_stepout_walk_is_the_same_however_it_is_scheduled(gpu_required, monkeypatch):
    """Speculation (shrink candidates ahead), the queue, the two-part launch, the full-solver instantiation, and the slim
    kernel with its full-solver finish of deferred walkers (whose basis the finishing slot rebuilds) change nothing."""
    with _model(3) as m:
        cube, theta, logl, lstar, chol = _start(m, 2600, seed=41, quantile=0.8)
        wr = wrapped_params(m.parnames)
        m.set_points_per_block(8)
        runs = {}
        for umax in (30.0, 1.0):
            m.set_slim_table_range(umax)
            for queue in ("0", "1", None):
                if queue is None:
                    monkeypatch.delenv("RVLL_WALK_QUEUE", raising=False)
                else:
                    monkeypatch.setenv("RVLL_WALK_QUEUE", queue)
                for spec in ("1", None):
                    if spec is None:
                        monkeypatch.delenv("RVLL_WALK_SPEC", raising=False)
                    else:
                        monkeypatch.setenv("RVLL_WALK_SPEC", spec)
                    runs[(umax, queue, spec)] = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=13, seed=5, **SO)
        monkeypatch.delenv("RVLL_WALK_SPEC", raising=False)
        monkeypatch.delenv("RVLL_WALK_QUEUE", raising=False)
        m.set_slim_table_range(30.0)
        monkeypatch.setenv("RVLL_WALK_FAT", "1")
        fat = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=13, seed=5, **SO)
        monkeypatch.setenv("RVLL_WALK_PARTS", "1")
        fat_one = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=13, seed=5, **SO)
    ref = runs[(30.0, "0", "1")]
    for key, got in runs.items():
        assert _same(got, ref), key
    assert _same(fat, ref) and _same(fat_one, ref)


def test_stepout_sharded_walk_draws_what_the_unsharded_walk_draws(gpu_required):
    from evidence_amd.sharded import partition
    with _model(3) as m:
        cube, theta, logl, lstar, chol = _start(m, 900, seed=31)
        wr = wrapped_params(m.parnames)
        full = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=7, seed=6, **SO)
        parts = [m.slice_walk(cube[lo:hi], theta[lo:hi], logl[lo:hi], lstar, chol, wr, nsteps=7, seed=6, walker_base=lo, **SO)
                 for lo, hi in partition(len(cube), 3)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), full[0])
    assert np.array_equal(np.concatenate([p[2] for p in parts]), full[2])
    assert sum(p[3] for p in parts) == full[3]


def test_stepout_run_mode_is_each_run_alone(gpu_required):
    with _model(3) as m:
        cube, theta, logl, lstar, chol = _start(m, 1200, seed=7)
        wr = wrapped_params(m.parnames)
        k = len(cube)
        run_start = np.array([0, k // 3, k // 2, k], dtype=np.int64)
        lst = np.array([lstar, lstar - 1.0, lstar + 0.0])
        chols = np.stack([chol, 0.5 * chol, chol])
        seeds = [3, 4, 5]
        both = m.slice_walk_runs(cube, theta, logl, run_start, lst, chols, wr, nsteps=8, seeds=seeds, **SO)
        steps = m.slice_walk_runs(cube, theta, logl, run_start, lst, chols, wr, nsteps=[8, 3, 5], seeds=seeds, **SO)
        for r, ns in enumerate((8, 3, 5)):
            sl = slice(run_start[r], run_start[r + 1])
            alone = m.slice_walk(cube[sl], theta[sl], logl[sl], lst[r], chols[r], wr, nsteps=8, seed=seeds[r], **SO)
            assert _same((both[0][sl], both[1][sl], both[2][sl], both[3][r]), alone), r
            alone = m.slice_walk(cube[sl], theta[sl], logl[sl], lst[r], chols[r], wr, nsteps=ns, seed=seeds[r], **SO)
            assert _same((steps[0][sl], steps[1][sl], steps[2][sl], steps[3][r]), alone), r


def test_stepout_resident_runs_and_ensembles_keep_their_equalities(gpu_required):
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    rundict, datadict, priordict, fixed = read_config(cfg, nplanets=1)
    with GpuRVModel(fixed, datadict, list(priordict), priordict=priordict) as m:
        prior, loglike = make_ultranest_callbacks(m, vectorized=True)
        wrap = wrapped_params(m.parnames)
        kw = dict(nlive=200, kbatch=50, dlogz=0.5, wrapped=wrap, max_calls=3_000_000, nsteps=5 * m.ndim, **SO)
        walker = run_nested_slice(prior, loglike, m.ndim, seed=3, walker=m.slice_walk, **kw)
        resident = run_nested_slice(None, None, m.ndim, seed=3, live=m, live_chol="host", **kw)
        assert resident.logz == walker.logz and resident.ncall == walker.ncall
        assert np.array_equal(resident.samples, walker.samples)
        for clustering in (False, True):
            ens = run_nested_ensemble(None, None, m.ndim, [5, 6], live=m, clustering=clustering, **kw)
            alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, clustering=clustering, **kw) for s in (5, 6)]
            for e, a in zip(ens, alone):
                assert e.logz == a.logz and e.ncall == a.ncall and np.array_equal(e.samples, a.samples), clustering
        # PolyChord's stop rule on the resident ensemble: each run stops where its standalone run does
        pc = dict(kw, precision_criterion=0.01)
        ens = run_nested_ensemble(None, None, m.ndim, [7, 8], live=m, **pc)
        alone = [run_nested_slice(None, None, m.ndim, seed=s, live=m, **pc) for s in (7, 8)]
        host = run_nested_slice(None, None, m.ndim, seed=7, live=m, live_chol="host", **pc)
        walked = run_nested_slice(prior, loglike, m.ndim, seed=7, walker=m.slice_walk, **pc)
    for e, a in zip(ens, alone):
        assert e.logz == a.logz and e.niter == a.niter
    assert host.niter == walked.niter and host.logz == walked.logz


def test_stepout_refusals_and_a_chord_walk_after_a_stepout_walk(gpu_required, monkeypatch):
    with _model(3) as m:
        cube, theta, logl, lstar, chol = _start(m, 800, seed=9)
        wr = wrapped_params(m.parnames)
        lib, h = m._lib, m._h
        for kind, width in ((2, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf"))):
            assert lib.rvll_set_walk_proposal(h, kind, width) == -1, (kind, width)      # RVLL_E_INVALID
        with pytest.raises(ValueError):
            m.set_walk_proposal("slice")
        with pytest.raises(RvllError):                       # every parameter wrapped: nothing bounds the bracket
            m.slice_walk(cube, theta, logl, lstar, chol, np.ones(m.ndim, dtype=bool), nsteps=2, seed=1, **SO)
        monkeypatch.setenv("RVLL_WALK_ROWS", "1")
        with pytest.raises(RvllError):
            m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=9, seed=1, **SO)
        monkeypatch.delenv("RVLL_WALK_ROWS")
        # the rounds form is not taken: 8192 walkers, where a chord walk takes it by default
        big = np.repeat(cube, 8192 // len(cube) + 1, axis=0)[:8192]
        bt, bl = m.prior_loglike_batch(big)
        m.slice_walk(big, bt, bl, lstar, chol, wr, nsteps=2, seed=1, **SO)
        assert m.slice_walk_rounds() == 0
        m.set_walk_proposal("stepout", 0.5)
        so_set = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=5, seed=2)
        so_kw = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=5, seed=2, proposal="stepout", step_width=0.5)
        m.set_walk_proposal("chord")
        after = m.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=5, seed=2)
    with _model(3) as fresh:
        ref = fresh.slice_walk(cube, theta, logl, lstar, chol, wr, nsteps=5, seed=2)
    assert _same(so_set, so_kw) and not _same(so_set, ref)
    assert _same(after, ref)
