"""GPU: the rotation between Newton steps (rvll_math.h: rotate_mid, newton_next_sincos) — the device against the host build,
and the log-L kernels with it: a point's bits are its own whatever shares its wave, tile or launch, the checked loops give
the shortcut loop's bits, and parity with the oracle holds across the eccentricities where a solve's first step crosses the
rotation's bound."""
import numpy as np
import pytest

import golden
import rotate_cases as rc
from evidence_amd import GpuRVModel
from evidence_amd.synthetic import make_workload
from test_gpu_loglike import TOL, _synthetic_case

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

N_EPOCHS, N_POINTS = 70, 192              # 70 epochs: every wave of 64 items holds two points
# Eccentricities: the class bounds a rule by eccentricity would have (0.3, 0.6) and one ulp either side, the eccentricity at
# which the first step can reach pi/4 (e / sqrt(1 - e^2) = pi/4 at 0.6177) from both sides, and calm, high and wandering ones
ECCS = np.array([0.0, np.nextafter(0.3, 0), 0.3, np.nextafter(0.3, 1), 0.8, np.nextafter(0.6, 0), 0.6, np.nextafter(0.6, 1), 0.97,
                 0.617, 0.62])


def _case():
    """(table, parnames, fixed, theta): 3 planets, 2 instruments; planet p of row i at ECCS[(4 i + 3 p) mod 11], so that
    neighbouring rows — the two points of a wave — and the planets of a row differ in class."""
    rng = np.random.default_rng(363)
    table, free, fixed, ranges, _ = _synthetic_case(rng, N_EPOCHS, 3, 2, False, 0, False)
    theta = np.stack([rng.uniform(*ranges[nm], N_POINTS) for nm in free], axis=1)
    for p in (1, 2, 3):
        theta[:, free.index(f"planet{p}_ecc")] = ECCS[(4 * np.arange(N_POINTS) + 3 * p) % ECCS.size]
        theta[:, free.index(f"planet{p}_period")] = rng.uniform(2.0, 40.0, N_POINTS)          # many orbits: M covers every phase
    return table, free, fixed, theta


@pytest.fixture(scope="module")
def case():
    return _case()


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


def test_rotate_mid_device_equals_host_bit_for_bit(gpu_required):
    """debug-eval 36 / 37 on 4096 seeded (E, h), the end points, h = 0 and denormal h among them: the inline-asm chains of the
    device against the FMA calls of the host build."""
    hr = rc.host_lib()
    if hr is None:
        pytest.skip("hipcc not available")
    E, h = rc.single_vector()
    E, h = E[:4096], h[:4096]
    hs, hc = rc.rotate_mid(hr, E, h)
    w = make_workload(1)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        ds, dc = m.debug_eval(36, E, h), m.debug_eval(37, E, h)
    assert np.array_equal(_bits(ds), _bits(hs)) and np.array_equal(_bits(dc), _bits(hc))


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
    """The same rows at itmax = 10000 (the unchecked first eight steps), at itmax = 8 (the shortcut is off: the checked loop
    from its start) and in tiles that hold a row with a wide planet (|M| >= 2^48: the tile's checked loop), on the rows whose
    solves all settle within seven steps by the oracle's own counts: the same bits, and the oracle's flags."""
    table, free, fixed, theta = case
    ref, rflags, settled = oracle
    assert settled.sum() >= N_POINTS // 2
    wide_row = theta[0].copy()
    wide_row[free.index("planet2_ma0")] = 2.0 ** 50
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
    with GpuRVModel(fixed, table, free, itmax=8) as m:
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            got = m.log_likelihood_batch(theta, return_flags=True)
            assert np.array_equal(_bits(got[0][settled]), _bits(base[settled])), form
            assert np.array_equal(got[1][settled], flags[settled]), form
    assert np.array_equal(flags[settled], rflags[settled])


def test_parity_across_the_rotation_bound(gpu_required, case, oracle):
    table, free, fixed, theta = case
    ref, rflags, _ = oracle
    with GpuRVModel(fixed, table, free) as m:
        got, flags = m.log_likelihood_batch(theta, return_flags=True)
    err = golden.rel_err(got, ref)
    calm = theta[:, [free.index(f"planet{p}_ecc") for p in (1, 2, 3)]].max(axis=1) <= 0.95
    print(f"rotation-bound rows: max rel err {err.max():.2e}, calm rows ({int(calm.sum())}) {err[calm].max():.2e}")
    assert np.array_equal(flags, rflags)
    assert err.max() <= TOL, (float(err.max()), int(err.argmax()))
    assert calm.sum() >= N_POINTS // 2 and err[calm].max() <= 1e-13, float(err[calm].max())
