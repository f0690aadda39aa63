"""CPU: the Newton step's fused residuals (rvll_math.h: newton_residuals) as the host compiles them (tests/native/hostnewton.hip):
against 50-digit arithmetic, and the solver with them against the solver with the reference's separately rounded residuals."""
import numpy as np
import pytest

import newton_cases as nc
import rotate_cases as rc


@pytest.fixture(scope="module")
def hn():
    lib = nc.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


def test_fused_residuals_against_50_digit_arithmetic(hn):
    """1e5 seeded rows (E over +-1e4 and over +-10, e over [0, 0.99], the solver's own pair at E, M within 1e-3 of E - e s).
    f = fma(-e, s, E) - M rounds twice: within half an ulp of fma(-e, s, E) plus half an ulp of the result of the exact
    E - e s - M; f' = fma(-e, c, 1) rounds once: within half an ulp of the exact 1 - e c.  Neither is ever further from the exact
    value than the separately rounded form gets on the same rows (its worst case, taken per range of E: the error of f scales
    with ulp(E))."""
    from mpmath.libmp import fone, from_float, mpf_abs, mpf_mul, mpf_sub, round_nearest, to_float
    E, s, c, ecc, M = nc.residual_rows()
    f1, fp1 = nc.residuals(hn, E, s, c, ecc, M, nc.FUSED)
    f0, fp0 = nc.residuals(hn, E, s, c, ecc, M, nc.SEPARATE)
    n = E.size
    ef1, ef0, efp1, efp0, t = (np.empty(n) for _ in range(5))
    prec = 170                                                  # 50 digits and a few more (mpmath's kernel functions: three times the mpf class's rate)

    def sub(a, b):
        return mpf_sub(a, b, prec, round_nearest)

    def dist(x, exact):
        return to_float(mpf_abs(sub(from_float(x), exact)))

    rows = zip(E.tolist(), s.tolist(), c.tolist(), ecc.tolist(), M.tolist(), f1.tolist(), f0.tolist(), fp1.tolist(), fp0.tolist())
    for i, (Ev, sv, cv, ev, Mv, f1v, f0v, fp1v, fp0v) in enumerate(rows):
        e_mp = from_float(ev)
        tt = sub(from_float(Ev), mpf_mul(e_mp, from_float(sv), prec, round_nearest))
        xf, xfp = sub(tt, from_float(Mv)), sub(fone, mpf_mul(e_mp, from_float(cv), prec, round_nearest))
        t[i] = to_float(tt, rnd=round_nearest)
        ef1[i], ef0[i], efp1[i], efp0[i] = dist(f1v, xf), dist(f0v, xf), dist(fp1v, xfp), dist(fp0v, xfp)
    assert (ef1 <= 0.5 * np.spacing(np.abs(t)) + 0.5 * np.spacing(np.abs(f1))).all()
    assert (efp1 <= 0.5 * np.spacing(np.abs(fp1))).all()
    for name, rows in (("|E| <= 1e4", slice(0, n // 2)), ("|E| <= 10", slice(n // 2, n))):
        print(f"{name}: max |f - exact| fused {ef1[rows].max():.3e} separate {ef0[rows].max():.3e}; "
              f"max |f' - exact| fused {efp1[rows].max():.3e} separate {efp0[rows].max():.3e}; "
              f"f differs on {np.mean(f1[rows] != f0[rows]):.2e} of the rows, f' on {np.mean(fp1[rows] != fp0[rows]):.2e}")
        assert ef1[rows].max() <= ef0[rows].max()
        assert efp1[rows].max() <= efp0[rows].max()
    assert (f1 != f0).any() and (fp1 != fp0).any()              # (the two forms are not the same function)


def test_fused_against_separate_residuals_under_the_rotation_rule(hn):
    """rotate_cases.solve_sample(): 1e6 solves (e from cfg3's prior, M over +-1e4), tol 1e-4, the shipped pair rule in both: no
    solve takes another number of steps, and the roots are within 4 ulp(E).  Measured on this host build: 0 solves, 2.0 ulp
    (9.1e-13), 100 roots of 1e6 with other bits."""
    M, ecc = rc.solve_sample()
    k0, E0, _, _ = nc.solve(hn, M, ecc, nc.SEPARATE)
    k1, E1, _, _ = nc.solve(hn, M, ecc, nc.FUSED)
    differ = k0 != k1
    ulps = np.abs(E0 - E1) / np.spacing(np.abs(E0))
    print(f"1e6 solves: step count differs on {int(differ.sum())}; max |dE| {np.abs(E0 - E1).max():.3e} = {ulps.max():.1f} ulp(E); "
          f"roots with other bits {int((E0 != E1).sum())}; mean steps {k0.mean():.3f}")
    assert not differ.any(), np.flatnonzero(differ)[:8]
    assert ulps.max() <= 4.0, float(ulps.max())


@pytest.mark.parametrize("which", [0, 1], ids=["e0.9-0.9925_M10", "e0.95-0.9925_M100"])
def test_high_eccentricity_samples(hn, which):
    """1e6 seeded solves where Newton from E = M is least forgiving: the class "ends within kSafeSteps" / "goes on" — what decides
    whether the tile redoes a solve correctly rounded — differs on at most 3 solves (a cap: a one-ulp nudge of sin / cos, which
    the rotated pair already is, flips 1 in 3e6), and among the solves that end within eight steps in the same number of them
    (cos nu, sin nu) move by at most 1e-9.  Measured on this host build: 0 and 1 class flips; 1.3e-13 and 3.6e-11."""
    M, ecc = nc.high_ecc_sample(which)
    k0, _, c0, s0 = nc.solve(hn, M, ecc, nc.SEPARATE)
    k1, _, c1, s1 = nc.solve(hn, M, ecc, nc.FUSED)
    flips = int(((k0 <= 8) != (k1 <= 8)).sum())
    same = (k0 == k1) & (k0 <= 8)
    dc, ds = np.abs(c0 - c1)[same].max(), np.abs(s0 - s1)[same].max()
    print(f"sample {which}: <= 8 / > 8 class differs on {flips} of {M.size}; {int(same.sum())} solves of equal count <= 8: "
          f"max |d cos nu| {dc:.3e}, max |d sin nu| {ds:.3e}; step count differs on {int((k0 != k1).sum())}")
    assert same.sum() >= M.size // 2
    assert flips <= 3
    assert dc <= 1e-9 and ds <= 1e-9
