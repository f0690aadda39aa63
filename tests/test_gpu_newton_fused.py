"""GPU: the Newton step's fused residuals (rvll_math.h: newton_residuals) — the device against the host build, and the log-L
kernels with them: a point's bits are its own whatever shares its wave, tile or launch, the checked loops give the shortcut
loop's bits, the flags are the oracle's and parity holds, also where |M| is small and the eccentricity high.  And the decode
step's per-point sum as a property of the fp64 kernels alone: the reduced-precision kernels against their recorded bits."""
import hashlib

import numpy as np
import pytest

import golden
import newton_cases as nc
from evidence_amd import FLAG_WANDERED, GpuRVModel
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

N_POINTS = nc.N_POINTS


@pytest.fixture(scope="module", params=[1, 2, 3], ids=["np1", "np2", "np3"])
def case(request):
    return nc.gpu_case(request.param)


@pytest.fixture(scope="module")
def oracle(case):
    """(log-L, flags, settled): the oracle on the case's rows, and the rows whose solves all settle in at most seven steps."""
    from evidence_amd.layout import compile_layout
    from oracle.oracle import OracleModel
    table, free, fixed, theta = case
    om = OracleModel(compile_layout(free, fixed, table.insts, []), table)
    ref, rflags = om.loglike(theta, nthreads=8, return_flags=True)
    settled = np.array([om.iteration_counts(x).max() <= 7 for x in theta])
    return ref, rflags, settled


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_residuals_device_equals_host_bit_for_bit(gpu_required):
    """debug-eval 38 / 39 on 4096 seeded records (E, s, c, e, M), |E| up to 1e4 and up to 10: f and f' of the device against the
    host build's."""
    hn = nc.host_lib()
    if hn is None:
        pytest.skip("hipcc not available")
    rec = nc.residual_records()
    hf, hfp = nc.residuals(hn, *rec.T, nc.FUSED)
    w = make_workload(1)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        df, dfp = m.debug_eval(38, rec.reshape(-1))[::5], m.debug_eval(39, rec.reshape(-1))[::5]
    assert np.array_equal(_bits(df), _bits(hf)) and np.array_equal(_bits(dfp), _bits(hfp))
    sf, sfp = nc.residuals(hn, *rec.T, nc.SEPARATE)
    assert (sf != hf).any() and (sfp != hfp).any()          # (the records tell the two forms apart)


def test_bits_are_the_points_own(gpu_required, case):
    table, free, fixed, theta = case
    perm = np.random.default_rng(5).permutation(N_POINTS)
    with GpuRVModel(fixed, table, free) as m:
        base, flags = m.log_likelihood_batch(theta, return_flags=True)
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            for pb in (1, 2, 7):
                m.set_points_per_block(pb)
                got = m.log_likelihood_batch(theta, return_flags=True)
                assert np.array_equal(_bits(got[0]), _bits(base)) and np.array_equal(got[1], flags), (form, pb)
                got = m.log_likelihood_batch(theta[perm], return_flags=True)
                assert np.array_equal(_bits(got[0]), _bits(base[perm])) and np.array_equal(got[1], flags[perm]), (form, pb, "perm")
        m.set_points_per_block(0)
        m.set_kernel_form("auto")
        singles = [m.log_likelihood_batch(theta[i:i + 1], return_flags=True) for i in range(N_POINTS)]
    assert np.array_equal(_bits(np.concatenate([s[0] for s in singles])), _bits(base))
    assert np.array_equal(np.concatenate([s[1] for s in singles]), flags)
    assert np.isfinite(base).all()


def test_checked_loops_give_the_shortcut_loops_bits(gpu_required, case, oracle):
    """The same rows at itmax = 10000 (the unchecked first eight steps), at itmax = 9 (the shortcut loop, then one step of the
    second), at itmax = 8 (the shortcut is off: the checked loop from its start) and in tiles that hold a row with a wide planet
    (|M| >= 2^48: the tile's checked loop), on the rows whose solves all settle within seven steps by the oracle's own counts:
    the same bits, and the oracle's flags."""
    table, free, fixed, theta = case
    ref, rflags, settled = oracle
    assert settled.sum() >= N_POINTS // 3
    wide_row = theta[0].copy()
    wide_row[free.index("planet1_ma0")] = 2.0 ** 50
    mixed = np.concatenate([np.concatenate([theta[i:i + 7], wide_row[None]]) for i in range(0, N_POINTS, 7)])
    own = np.ones(mixed.shape[0], dtype=bool)
    own[7::8] = False                                   # every eighth row is the wide one ...
    own[-1] = False                                     # ... and so is the last (192 = 27 * 7 + 3)
    assert own.sum() == N_POINTS
    with GpuRVModel(fixed, table, free) as m:
        base, flags = m.log_likelihood_batch(theta, return_flags=True)
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            m.set_points_per_block(8)
            got = m.log_likelihood_batch(mixed, return_flags=True)
            assert np.array_equal(_bits(got[0][own][settled]), _bits(base[settled])), form
            assert np.array_equal(got[1][own][settled], flags[settled]), form
    for itmax in (8, 9):
        with GpuRVModel(fixed, table, free, itmax=itmax) as m:
            for form in ("tile", "cu"):
                m.set_kernel_form(form)
                got = m.log_likelihood_batch(theta, return_flags=True)
                assert np.array_equal(_bits(got[0][settled]), _bits(base[settled])), (form, itmax)
                assert np.array_equal(got[1][settled], flags[settled]), (form, itmax)
    assert np.array_equal(flags[settled], rflags[settled])


def test_flags_and_parity_with_the_oracle(gpu_required, case, oracle):
    """Every row carries the oracle's flags — RVLL_FLAG_WANDERED exactly where the reference's own iteration takes more than
    eight steps: the class the fused residuals must not move.  Rows whose eccentricities are all <= 0.8: 1e-13; every row
    without the flag: 1e-10."""
    table, free, fixed, theta = case
    ref, rflags, _ = oracle
    with GpuRVModel(fixed, table, free) as m:
        got, flags = m.log_likelihood_batch(theta, return_flags=True)
    err = golden.rel_err(got, ref)
    calm = theta[:, [i for i, nm in enumerate(free) if nm.endswith("_ecc")]].max(axis=1) <= 0.8
    kept = (flags & FLAG_WANDERED) == 0
    print(f"{len(free)} parameters: max rel err {err.max():.2e}; rows with e <= 0.8 ({int(calm.sum())}) {err[calm].max():.2e}; "
          f"rows that did not wander ({int(kept.sum())}) {err[kept].max():.2e}; the long-period rows {err[-nc.N_LONG:].max():.2e}")
    assert np.array_equal(flags, rflags)
    assert calm.sum() >= 8 and err[calm].max() <= 1e-13, float(err[calm].max())
    assert kept.sum() >= N_POINTS // 3 and err[kept].max() <= 1e-10, float(err[kept].max())


@pytest.mark.parametrize("precision", ["mixed", "fp32"])
def test_reduced_precision_kernels_keep_their_bits(gpu_required, precision):
    """The reduced-precision kernels do not read the decode step's per-point sum and no longer carry its loop: log-L of a
    five-planet, 64-epoch, 130-point model at 1, 2, 7 points a block and at the default, against the bits recorded with the
    library of the commit before (tests/golden/loglike_reduced_np5.npz: one array per launch shape — the float sums of these
    kernels depend on the points a block, 34 of 130 rows at 7 have the default's bits — and a hash of the rows)."""
    table, free, fixed, theta = nc.reduced_case()
    z = np.load(golden.GOLDEN / "loglike_reduced_np5.npz")
    assert hashlib.sha256(np.ascontiguousarray(theta).tobytes()).digest() == z["theta_sha256"].tobytes()
    with GpuRVModel(fixed, table, free, precision=precision) as m:
        got = m.log_likelihood_batch(theta)
        assert np.array_equal(_bits(got), _bits(z[precision])), "default"
        for pb in (1, 2, 7):
            m.set_points_per_block(pb)
            assert np.array_equal(_bits(m.log_likelihood_batch(theta)), _bits(z[f"{precision}_pb{pb}"])), pb
