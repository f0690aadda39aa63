"""CPU: the simulated-shrinkage definition (evidence_amd/shrinkage.py).  Its expected mode gives back every driver's own
logz, information and logwt, so the (nlive, kbatch) schedule the results record is the one they died by; the replicate
spread of one run is the spread of ln Z over independent perfect nested-sampling runs, with one and with many deaths per
iteration; the draws are rvll_math.h's uniform01; malformed inputs are refused."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from evidence_amd import run_nested_ensemble, shrinkage
from evidence_amd.clustering import keep_words
from evidence_amd.nested import run_nested, run_nested_slice
from test_nested_ensemble_host import _WalkerRuns
from test_nested_resident_ensemble_host import _OneRun, _Runs

HERE = Path(__file__).resolve().parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def prior(cube):
    return -10.0 + 20.0 * cube


def loglike(x):
    return -0.5 * np.sum(x * x, axis=1)


def _expected_matches(res):
    """Expected-mode replicates of one result against its own logz / information / logwt."""
    assert res.nlive is not None and res.kbatch is not None
    logz, info, w = shrinkage.replicates([res], nsamples=2, mode="expected", return_logwt=True)
    assert np.all(np.abs(logz - res.logz) <= 1e-10), (logz, res.logz)
    assert np.all(np.abs(info - res.information) <= 1e-10), (info, res.information)
    keep = res.logwt > -50
    assert keep.sum() > 10
    assert np.abs(w[0][:, keep] - res.logwt[keep]).max() <= 1e-10


def test_expected_mode_reproduces_run_nested():
    res = run_nested(prior, loglike, 2, nlive=100, seed=4)
    assert (res.nlive, res.kbatch) == (100, 1)
    _expected_matches(res)


def test_expected_mode_reproduces_run_nested_budget_cut():
    # max_calls ends the run mid-replacement: one live point fewer than nlive at the end (m = nlive - 1)
    res = run_nested(prior, loglike, 2, nlive=60, seed=5, max_calls=2000)
    assert len(res.logl) - res.niter == 59
    _expected_matches(res)


@pytest.mark.parametrize("kbatch", [1, 7, 25])
def test_expected_mode_reproduces_run_nested_slice(kbatch):
    res = run_nested_slice(prior, loglike, 2, nlive=100, kbatch=kbatch, nsteps=4, seed=kbatch, max_calls=60_000)
    assert (res.nlive, res.kbatch) == (100, kbatch) and res.niter % kbatch == 0
    _expected_matches(res)


def test_expected_mode_reproduces_the_slice_default_kbatch():
    res = run_nested_slice(prior, loglike, 2, seed=3, max_calls=60_000)
    assert res.kbatch == res.nlive // 4 == 12
    _expected_matches(res)


def test_expected_mode_reproduces_the_host_ensemble():
    got = run_nested_ensemble(prior, loglike, 2, [1, 2, 3], nlive=120, kbatch=10, nsteps=3, dlogz=0.1, max_calls=400_000,
                              walker_runs=_WalkerRuns())
    for res in got:
        assert (res.nlive, res.kbatch) == (120, 10)
        _expected_matches(res)
    logz, info = shrinkage.replicates(got, nsamples=1, mode="expected")
    assert np.allclose(logz[:, 0], [g.logz for g in got], rtol=0, atol=1e-10)


def test_expected_mode_reproduces_the_resident_ensemble():
    kw = dict(nlive=120, kbatch=10, nsteps=3, dlogz=0.1, max_calls=400_000)
    got = run_nested_ensemble(None, None, 2, [5, 6, 7], live=_Runs(), **kw)
    got.append(run_nested_slice(None, None, 2, seed=8, live=_OneRun(), **kw))      # the one-run resident live set
    for res in got:
        assert (res.nlive, res.kbatch) == (120, 10)
        _expected_matches(res)


def test_results_without_a_schedule_need_overrides():
    res = run_nested_slice(prior, loglike, 2, nlive=60, kbatch=6, nsteps=3, seed=1, max_calls=20_000)
    res.nlive = res.kbatch = None
    with pytest.raises(ValueError, match="nlive"):
        shrinkage.replicates([res], nsamples=2)
    logz, _ = shrinkage.replicates([res], nsamples=2, mode="expected", nlive=60, kbatch=6)
    assert np.all(np.abs(logz - res.logz) <= 1e-10)


# ---- the spread ---------------------------------------------------------------------------------------------------------
def _log_like_of_x(logx):
    return -50.0 * np.exp(logx)                  # L(X) = exp(-50 X): a 2-D Gaussian in its prior volume; Z = (1 - e^-50) / 50


def _perfect_run(rng, nlive, kbatch, iters):
    """Exact nested sampling of L(X) with an explicit live set: each iteration kills the kbatch live points of largest X
    (lowest L) in order and draws kbatch replacements uniformly in X below the last of them.  Returns (logl, n_dead)."""
    logx = np.log(rng.random(nlive))
    dead = []
    for _ in range(iters):
        order = np.argsort(-logx)
        kill = order[:kbatch]
        dead.append(logx[kill])
        logx[kill] = logx[kill[-1]] + np.log(rng.random(kbatch))
    dead = np.concatenate(dead)
    return np.concatenate([_log_like_of_x(dead), _log_like_of_x(logx)]), dead.size


@pytest.mark.parametrize("kbatch", [50, 1])
def test_replicate_spread_is_the_spread_over_runs(kbatch):
    nlive, nruns = 200, 300
    iters = 2000 // kbatch                         # logX down to ~ -10: the posterior bulk (X ~ 1/50) well passed
    rng = np.random.default_rng(11 + kbatch)
    runs = [_perfect_run(rng, nlive, kbatch, iters) for _ in range(nruns)]
    logl = np.concatenate([r[0] for r in runs])
    run_start = np.concatenate([[0], np.cumsum([len(r[0]) for r in runs])])
    n_dead = [r[1] for r in runs]
    est, _ = shrinkage.replicates_arrays(logl, run_start, n_dead, [nlive] * nruns, [kbatch] * nruns, range(nruns), 1,
                                         mode="expected")
    truth = np.std(est[:, 0], ddof=1)
    assert abs(np.mean(est[:, 0]) - np.log((1 - np.exp(-50.0)) / 50.0)) < 3 * truth / np.sqrt(nruns) + 0.01
    # the replicate spread (S = 2000) of each of the first 16 runs, as an rms over them
    k = 16
    reps, _ = shrinkage.replicates_arrays(logl[:run_start[k]], run_start[:k + 1], n_dead[:k], [nlive] * k, [kbatch] * k,
                                          range(k), 2000)
    spread = np.sqrt(np.mean(np.var(reps, axis=1, ddof=1)))
    assert 0.8 <= spread / truth <= 1.25, (spread, truth)
    if kbatch > 1:
        # the batch schedule matters: a constant live count (one death per iteration) understates the scatter
        flat, _ = shrinkage.replicates_arrays(logl[:run_start[k]], run_start[:k + 1], n_dead[:k], [nlive] * k, [1] * k,
                                              range(k), 2000)
        flat = np.sqrt(np.mean(np.var(flat, axis=1, ddof=1)))
        assert flat < spread and abs(np.log(spread / truth)) < abs(np.log(flat / truth)), (spread, flat, truth)


# ---- draws, blocks, validation ----------------------------------------------------------------------------------------
def _splitmix_u(seed, j):
    z = (seed + 0x9E3779B97F4A7C15 * (j + 1)) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    return float((z ^ (z >> 31)) >> 11) * 2.0 ** -53


def test_draws_are_the_uniform01_of_rvll_math():
    seeds = [0, 1, 2 ** 64 - 1, 0xD1B54A32D192ED03 * 3 % 2 ** 64, 123456789]
    u = shrinkage.uniform01(seeds, 300)
    for i, s in enumerate(seeds):
        assert [_splitmix_u(s, j) for j in range(300)] == list(u[i])
        assert np.array_equal(u[i], (keep_words(s, 300) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
    with np.errstate(over="ignore"):
        want = np.uint64(5) + np.uint64(shrinkage.SEED_MUL) * np.arange(4, dtype=np.uint64)
    assert np.array_equal(shrinkage.replicate_seeds(5, 4), want)


def test_draws_match_the_compiled_header():
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    src, lib = HERE / "native" / "shrinkuniform.hip", HERE / "native" / "libshrinkuniform.so"
    hdr = HERE.parent / "evidence_amd" / "csrc" / "rvll_math.h"
    if not lib.exists() or lib.stat().st_mtime < max(src.stat().st_mtime, hdr.stat().st_mtime):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{hdr.parent}", str(src), "-o", str(lib)], check=True)
    su = C.CDLL(str(lib))
    for seed in (0, 42, 2 ** 63 + 12345, int(shrinkage.replicate_seeds(9, 1000)[999])):
        out = np.empty(5000)
        su.su_uniform01(C.c_ulonglong(seed), C.c_long(out.size), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert np.array_equal(out, shrinkage.uniform01([seed], out.size)[0])


def _ragged(rng):
    runs = [(0, 30, 3, 1), (240, 200, 40, 200), (90, 12, 1, 12), (1504, 64, 16, 64)]    # (n_dead, nlive, kbatch, m)
    logl, meta = [], []
    for n_dead, nlive, kbatch, m in runs:
        ll = np.sort(rng.normal(0, 3, n_dead + m))
        ll[:3] = -1e30
        logl.append(ll)
        meta.append((n_dead, nlive, kbatch))
    return (np.concatenate(logl), np.concatenate([[0], np.cumsum([len(x) for x in logl])]),
            *[list(v) for v in zip(*meta)])


def test_blocks_do_not_change_the_bits(monkeypatch):
    logl, run_start, n_dead, nlive, kbatch = _ragged(np.random.default_rng(2))
    big = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, [1, 2, 3, 4], 9, return_logwt=True)
    monkeypatch.setattr(shrinkage, "_BLOCK_ELEMS", 1000)
    small = shrinkage.replicates_arrays(logl, run_start, n_dead, nlive, kbatch, [1, 2, 3, 4], 9, return_logwt=True)
    assert np.array_equal(big[0], small[0]) and np.array_equal(big[1], small[1])
    assert all(np.array_equal(a, b) for a, b in zip(big[2], small[2]))
    # a run alone is the run inside the batch
    alone = shrinkage.replicates_arrays(logl[run_start[1]:run_start[2]], [0, run_start[2] - run_start[1]], n_dead[1:2],
                                        nlive[1:2], kbatch[1:2], [2], 9)
    assert np.array_equal(alone[0][0], big[0][1]) and np.array_equal(alone[1][0], big[1][1])
    for w in big[2]:
        assert np.allclose(np.logaddexp.reduce(w, axis=1), 0.0, atol=1e-12)
    assert np.all(big[1][0] == 0.0)                 # no dead points: no information


def test_logz_error_is_the_replicate_spread():
    res = run_nested_slice(prior, loglike, 2, nlive=80, kbatch=8, nsteps=3, seed=2, max_calls=40_000)
    err = shrinkage.logz_error([res], nsamples=400, seed=3)
    logz, _ = shrinkage.replicates([res], nsamples=400, seed=3)
    assert err.shape == (1,) and err[0] == np.std(logz[0]) and 0.5 < err[0] / res.logzerr < 2.0
    assert not np.array_equal(shrinkage.replicates([res], nsamples=4, seed=4)[0], logz[:, :4])


BAD = [
    (dict(run_start=[0, 5, 9]), "run_start"),                      # does not add up to the rows
    (dict(run_start=[1, 5, 10]), "run_start"),
    (dict(run_start=[0, 6, 4, 10], n_dead=[2, 0, 2], nlive=[5] * 3, kbatch=[1] * 3, seeds=[0, 1, 2]), "run_start"),
    (dict(n_dead=[-1, 2]), "n_dead"),
    (dict(n_dead=[3, 2]), "multiple of kbatch"),
    (dict(kbatch=[5, 1]), "kbatch"),
    (dict(kbatch=[0, 1]), "kbatch"),
    (dict(n_dead=[6, 2], kbatch=[2, 1]), "final live row"),           # m = 0
    (dict(seeds=[1]), "seeds"),
    (dict(nsamples=0), "nsamples"),
    (dict(nsamples=-3), "nsamples"),
    (dict(mode="median"), "mode"),
]


@pytest.mark.parametrize("change,match", BAD)
def test_malformed_inputs_are_refused(change, match):
    kw = dict(logl=np.zeros(10), run_start=[0, 6, 10], n_dead=[4, 2], nlive=[5, 5], kbatch=[2, 1], seeds=[0, 1],
              nsamples=3, mode="random")
    kw.update(change)
    with pytest.raises(ValueError, match=match):
        shrinkage.replicates_arrays(**kw)
