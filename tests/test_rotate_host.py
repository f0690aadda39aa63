"""CPU: the rotation between Newton steps (rvll_math.h: rotate_mid, newton_next_sincos) as the host compiles it
(tests/native/hostrotate.hip): its error against mpmath, and the solver with it against the solver without."""
import numpy as np
import pytest

import rotate_cases as rc


@pytest.fixture(scope="module")
def hr():
    lib = rc.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


def test_rotate_mid_against_mpmath(hr):
    """The pair of sincos_f64 at 1e5 seeded E over +-1e4, rotated by h over (0, pi/4] of both signs — end points, h = 0 and
    denormal h included — against sin / cos of the exact E + h: the maxima measured with this very vector
    (profiles/math_primitives.txt), rounded up to the next half unit of 2^-53.  The pair itself carries up to 1.2."""
    assert hr.hr_rotate_mid_max() == rc.MID_MAX
    E, h = rc.single_vector()
    s, c = rc.rotate_mid(hr, E, h)
    es, ec = rc.err_vs_mpmath(E, h, s, c)
    print(f"host rotate_mid: sin {es:.3f} cos {ec:.3f} (2^-53), n = {E.size}")
    assert es <= rc.half_up(rc.ROTATE_MID_MEASURED[0]) and ec <= rc.half_up(rc.ROTATE_MID_MEASURED[1]), (es, ec)
    zero = h == 0
    s0, c0 = rc.rotate_mid(hr, E[zero], np.zeros((int(zero.sum()), 0)))
    assert np.array_equal(s[zero], s0) and np.array_equal(c[zero], c0)            # h = 0 leaves the pair as it is


def test_seven_rotations_in_a_row_against_mpmath(hr):
    """The most the shortcut loop can make (eight evaluations), every step as large as the bound allows on a third of the rows:
    against sin / cos of the exact E + h1 + .. + h7.  (A solve's steps shrink quadratically: this is the worst case by far.)"""
    E, H = rc.chain_vector()
    s, c = rc.rotate_mid(hr, E, H)
    es, ec = rc.err_vs_mpmath(E, H, s, c)
    print(f"host rotate_mid x 7: sin {es:.3f} cos {ec:.3f} (2^-53), n = {E.size}")
    assert es <= rc.half_up(rc.ROTATE_MID_CHAIN_MEASURED[0]) and ec <= rc.half_up(rc.ROTATE_MID_CHAIN_MEASURED[1]), (es, ec)


def test_no_calm_solve_changes_its_step_count(hr):
    """1e6 seeded solves (e from cfg3's prior, M over +-1e4, tol 1e-4, itmax 10000), the full pair at every step against
    newton_next_sincos: no solve with e <= 0.95 takes another number of steps (a flip moves log-L by ~1e-9), and where the count
    is the same the roots are within a few ulps of E (recorded: profiles/r05_newton_rotation.txt)."""
    M, ecc = rc.solve_sample()
    k0, E0 = rc.solve(hr, M, ecc, 0)
    k1, E1 = rc.solve(hr, M, ecc, 1)
    differ = k0 != k1
    calm = ecc <= 0.95
    same = ~differ
    print(f"1e6 solves: step count differs on {int(differ.sum())} ({int((differ & calm).sum())} with e <= 0.95); where it does not, "
          f"max |dE| {np.abs(E0 - E1)[same].max():.3e} = {(np.abs(E0 - E1)[same] / np.spacing(np.abs(E0[same]))).max():.1f} ulp(E); "
          f"mean steps {k0.mean():.3f}")
    assert not (differ & calm).any(), np.flatnonzero(differ & calm)[:8]
    # NaN and an absurd step take the full route: the same bits as the solver without the rotation
    bad_M = np.array([np.nan, 2.0 ** 60, -2.0 ** 52, 1e300])
    for rule_ecc in (0.1, 0.99):
        a, b = rc.solve(hr, bad_M, np.full(4, rule_ecc), 0, itmax=20), rc.solve(hr, bad_M, np.full(4, rule_ecc), 1, itmax=20)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
