"""GPU: the one-division log-L item (rvll_math.h: ItemPool; rvll_tile.h: eval_item, tile_decode) in the kernels: every
instantiation of the planet loop (compile-time 1 / 3, the run-time loop), with and without drift and linear terms, epoch
counts either side of a wave round, tiles of one point to several waves of planets in the decode step — against the oracle,
and the same bits whatever shares a point's wave, tile or launch; the nu = 0 planet inside the pool; the NaN mark of a
wandering solve through the pooled numerator; a non-finite row."""
import numpy as np
import pytest

import golden
from evidence_amd import GpuRVModel, FLAG_NONCONVERGED, FLAG_WANDERED
from test_gpu_loglike import TOL, _synthetic_case

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

ECCS = np.array([0.0, 0.6, 0.8, 0.3, 0.05])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case(seed, n_epochs, nplanets, drift, nlin, npts):
    """Two instruments, every parameter free; planet p of row i at ECCS[(i + 2 p) mod 5] (0, 0.6 and 0.8 among them), short
    periods (many orbits: every phase)."""
    rng = np.random.default_rng(seed)
    table, free, fixed, ranges, linpar = _synthetic_case(rng, n_epochs, nplanets, min(2, n_epochs), drift, nlin, False)
    theta = np.stack([rng.uniform(*ranges[nm], npts) for nm in free], axis=1)
    for p in range(1, nplanets + 1):
        theta[:, free.index(f"planet{p}_ecc")] = ECCS[(np.arange(npts) + 2 * p) % ECCS.size]
        theta[:, free.index(f"planet{p}_period")] = rng.uniform(2.0, 40.0, npts)
    return table, free, fixed, theta, linpar


def _oracle(m, table, linpar, theta):
    from oracle.oracle import OracleModel
    layout = m.layout
    series = np.stack([linpar[k] for k in layout.linpar_names]) if layout.linpar_names else None
    return OracleModel(layout, table, series).loglike(theta, nthreads=8, return_flags=True)


# planets 0 1 2 3 5; epochs 1 63 64 65 70 128 200 (a wave round holds 64 items); 1 2 7 65 130 points a launch (65 points of
# three planets: four waves of the decode step; 130 of five: eleven); drift + a linear term on and off for every planet count
@pytest.mark.parametrize("n_epochs,nplanets,extras,npts", [
    (1, 1, False, 130), (63, 3, False, 65), (64, 3, True, 7), (65, 2, False, 130), (70, 3, False, 130), (128, 5, True, 65),
    (200, 3, False, 65), (200, 0, False, 7), (70, 0, True, 65), (65, 1, True, 2), (128, 1, False, 1), (200, 2, True, 7),
    (63, 5, False, 130), (70, 3, True, 2), (200, 5, False, 1),
])
def test_parity_and_bits_in_every_instantiation(gpu_required, n_epochs, nplanets, extras, npts):
    table, free, fixed, theta, linpar = _case(620 + n_epochs + nplanets, n_epochs, nplanets, extras, 1 if extras else 0, npts)
    perm = np.random.default_rng(6).permutation(npts)
    with GpuRVModel(fixed, table, free, linpar_dict=linpar or None) as m:
        base, flags = m.log_likelihood_batch(theta, return_flags=True)
        ref, rflags = _oracle(m, table, linpar, theta)
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
        singles = np.concatenate([m.log_likelihood_batch(theta[i:i + 1]) for i in range(min(npts, 65))])
    err = golden.rel_err(base, ref)
    print(f"{n_epochs} epochs, {nplanets} planets, extras {extras}, {npts} points: max rel err {err.max():.2e}")
    assert np.array_equal(_bits(singles), _bits(base[:singles.size]))
    assert np.isfinite(base).all() and np.array_equal(flags, rflags)
    assert err.max() <= 1e-13, (float(err.max()), int(err.argmax()))


def test_a_planet_out_of_steps_sits_inside_the_pool(gpu_required):
    """itmax = 5, three planets: the middle one at e = 0.7 runs out of steps at some epoch and keeps nu = 0 from there on
    (trueanomaly.c:32-33) — it joins the pool as A / 1 — while the outer two (e <= 0.1: three steps) converge at every epoch.  The
    oracle's value at the bar of tests/test_gpu_solver_settings.py's parity group, its flags, the same bits in both forms."""
    table, free, fixed, theta, linpar = _case(640, 200, 3, False, 0, 65)
    theta[:, free.index("planet1_ecc")] = 0.1
    theta[:, free.index("planet3_ecc")] = 0.0
    theta[:, free.index("planet2_ecc")] = 0.7
    mild = theta.copy()
    mild[:, free.index("planet2_ecc")] = 0.1
    with GpuRVModel(fixed, table, free, itmax=5) as m:
        base, flags = m.log_likelihood_batch(theta, return_flags=True)
        ref, rflags = _oracle(m, table, linpar, theta)
        _, mild_flags = m.log_likelihood_batch(mild, return_flags=True)
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            for pb in (1, 7):
                m.set_points_per_block(pb)
                got = m.log_likelihood_batch(theta, return_flags=True)
                assert np.array_equal(_bits(got[0]), _bits(base)) and np.array_equal(got[1], flags), (form, pb)
    err = golden.rel_err(base, ref)
    print(f"middle planet out of steps: max rel err {err.max():.2e}, flags {np.unique(flags).tolist()}")
    assert not mild_flags.any()                                    # the outer two, and the middle one at their eccentricity, converge
    assert np.array_equal(flags, rflags) and ((flags & FLAG_NONCONVERGED) != 0).all()
    assert err.max() <= TOL, (float(err.max()), int(err.argmax()))


def test_a_wandering_solve_is_marked_through_the_pool_and_redone(gpu_required):
    """One row with a planet at e = 0.99 among calm ones, 70 epochs (its items share their waves with both neighbours'): some
    solve of it wanders, the first pass leaves that item NaN through the pooled numerator, the redo pass finds it — WANDERED,
    within 1e-10 of the oracle — and the other rows have the bits of a launch without it."""
    table, free, fixed, theta, linpar = _case(650, 70, 3, False, 0, 33)
    row = 16
    calm_row = theta[row].copy()
    theta[row, free.index("planet2_ecc")] = 0.99
    theta[row, free.index("planet2_period")] = 2.5               # 70 epochs over ~1200 orbits: some phase near periastron
    without = theta.copy()
    without[row] = calm_row
    others = np.arange(theta.shape[0]) != row
    with GpuRVModel(fixed, table, free) as m:
        ref, rflags = _oracle(m, table, linpar, theta)
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            got, flags = m.log_likelihood_batch(theta, return_flags=True)
            base, bflags = m.log_likelihood_batch(without, return_flags=True)
            err = golden.rel_err(got, ref)
            print(f"{form}: wandering row {err[row]:.2e}, the others {err[others].max():.2e}, flags of the row {int(flags[row])}")
            assert np.isfinite(got).all()
            assert flags[row] & FLAG_WANDERED and np.array_equal(flags, rflags)
            assert err.max() <= 1e-10, float(err.max())
            assert np.array_equal(_bits(got[others]), _bits(base[others])) and not flags[others].any() and not bflags.any()


def test_a_non_finite_row_disturbs_nothing(gpu_required):
    table, free, fixed, theta, linpar = _case(660, 70, 3, True, 1, 65)
    bad = theta.copy()
    bad[5, free.index("planet2_k1")] = np.nan
    bad[40, free.index("i0_offset")] = np.inf
    bad[41, free.index("planet3_period")] = np.nan
    clean = np.ones(65, dtype=bool)
    clean[[5, 40, 41]] = False
    with GpuRVModel(fixed, table, free, linpar_dict=linpar or None) as m:
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            base = m.log_likelihood_batch(theta)
            got = m.log_likelihood_batch(bad)
            assert not np.isfinite(got[~clean]).any(), form
            assert np.array_equal(_bits(got[clean]), _bits(base[clean])), form
