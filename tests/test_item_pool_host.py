"""CPU: the one-division log-L item (rvll_math.h: ItemPool, pool_add, pool_chi2) as the host compiles it
(tests/native/hostitem.hip): the pooled routine against a 50-digit evaluation of sum_p n_p / d_p and of res^2 / (2 var), its
special cases bit for bit, and a whole log-L through it against the oracle at the bars of tests/test_gpu_loglike.py.

The bounds of the first test are worked out, not measured (u = 2^-53, Q = sum_p |n_p / d_p|, first order in u):
  D_k = D_{k-1} d_k carries k - 1 roundings; N_k = fma(n_k, D_{k-1}, fl(N_{k-1} d_k)) adds, relative to D_k, at most
  (k - 2) u |q_k| (the error of D_{k-1}), u |S_{k-1}| (the product) and u |S_k| (the FMA): |N / D - S| <= 3 Np u Q from N and
  (Np - 1) u |S| from D, together <= 4 Np u Q;
  T = fma(R, D, -N) adds u |T|: T / D is within delta = (4 Np + 2) u (|R| + Q) of res = R - S;
  T T, D D, (2 var)(D D) and the quotient are four roundings more: chi is within (2 |res| delta + delta^2) / (2 var) + 5 u chi."""
import numpy as np
import pytest

import golden
import item_pool_cases as ic
from evidence_amd.synthetic import make_workload


@pytest.fixture(scope="module")
def hi():
    lib = ic.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("npl", [1, 2, 3, 5])
def test_pool_against_exact_quotients(hi, npl):
    import mpmath
    num, den, R, var = ic.quotient_rows(npl)
    chi, N, D = ic.pool(hi, num, den, R, var)
    old = ic.separate(hi, num, den, R, var)
    S, chi_x, mag = ic.exact(num, den, R, var)
    worst_sum = worst_chi = worst_old = 0.0
    with mpmath.workdps(50):
        for i in range(len(S)):
            q_mag = mag[i] - abs(mpmath.mpf(float(R[i])))
            err_sum = abs(mpmath.mpf(float(N[i])) / mpmath.mpf(float(D[i])) - S[i])
            assert err_sum <= (4 * npl + 1) * ic.U * q_mag, (i, float(err_sum), float(q_mag))
            delta = (4 * npl + 2) * ic.U * mag[i]
            res = abs(mpmath.mpf(float(R[i])) - S[i])
            bound = (2 * res * delta + delta * delta) / (2 * mpmath.mpf(float(var[i]))) + 5 * ic.U * chi_x[i]
            err_chi = abs(mpmath.mpf(float(chi[i])) - chi_x[i])
            assert err_chi <= bound, (i, float(err_chi), float(bound))
            scale = (2 * res + ic.U * mag[i]) * ic.U * mag[i] / (2 * mpmath.mpf(float(var[i]))) + ic.U * chi_x[i]
            worst_sum = max(worst_sum, float(err_sum / (ic.U * q_mag)))
            worst_chi = max(worst_chi, float(err_chi / scale))
            worst_old = max(worst_old, float(abs(mpmath.mpf(float(old[i])) - chi_x[i]) / scale))
    same = float((_bits(chi) == _bits(old)).mean())
    print(f"Np = {npl}: N / D within {worst_sum:.2f} u Q of the exact sum; item within {worst_chi:.2f} of its u-scale "
          f"(one quotient per planet: {worst_old:.2f}); {same:.1%} of the rows the same bits either way")


@pytest.mark.parametrize("npl", [1, 2, 3, 5])
def test_a_planet_at_nu_0_joins_as_a_over_1(hi, npl):
    """den = 1 in each position in turn: D is the product of the OTHER denominators in planet order, bit for bit (a
    multiplication by 1 is exact), and with only such planets the item is the separate arithmetic's: N = sum of the A."""
    num, den, R, var = (a.copy() for a in ic.quotient_rows(npl))
    for pos in range(npl):
        d = den.copy()
        d[:, pos] = 1.0
        _, _, D = ic.pool(hi, num, d, R, var)
        want = np.ones(len(R))
        first = True
        for k in range(npl):
            if k == pos:
                continue
            want = d[:, k].copy() if first else want * d[:, k]
            first = False
        assert np.array_equal(_bits(D), _bits(want)), pos
    ones = np.ones_like(den)
    chi, N, D = ic.pool(hi, num, ones, R, var)
    ksum = num[:, 0].copy()
    for k in range(1, npl):
        ksum = ksum + num[:, k]
    res = R - ksum
    assert np.array_equal(_bits(D), _bits(np.ones(len(R)))) and np.array_equal(_bits(N), _bits(ksum))
    assert np.array_equal(_bits(chi), _bits(res * res / (2 * var)))


@pytest.mark.parametrize("npl", [1, 2, 3, 5])
def test_nan_numerator_propagates(hi, npl):
    """The first pass marks an item with a wandering solve by a NaN numerator: whatever the position, the item is NaN, and no
    other row moves."""
    num, den, R, var = (a.copy() for a in ic.quotient_rows(npl, 400))
    base, _, _ = ic.pool(hi, num, den, R, var)
    assert np.isfinite(base).all()
    for pos in range(npl):
        n2 = num.copy()
        n2[pos::7, pos] = np.nan
        got, _, _ = ic.pool(hi, n2, den, R, var)
        marked = np.isnan(n2).any(axis=1)
        assert np.isnan(got[marked]).all() and np.array_equal(_bits(got[~marked]), _bits(base[~marked]))


def test_no_planet_is_the_separate_form_bit_for_bit(hi):
    rng = np.random.default_rng(610)
    R = np.concatenate([rng.uniform(-50, 50, 1000), [0.0, -0.0, 1e-300, -1e300, np.inf, np.nan]])
    var = np.concatenate([rng.uniform(0.25, 2500.0, 1000), [1.0, 1.0, 2.0, 3.0, 1.0, 1.0]])
    empty = np.empty((R.size, 0))
    chi, N, D = ic.pool(hi, empty, empty, R, var)
    with np.errstate(all="ignore"):
        want = R * R / (2 * var)
    assert np.array_equal(_bits(chi), _bits(want))
    assert np.array_equal(_bits(chi), _bits(ic.separate(hi, empty, empty, R, var)))


def test_whole_loglike_against_the_oracle(hi):
    """20 000 prior draws of cfg3 (3 planets, 200 epochs): the host build of the decode step, the solver and the pooled item
    against the oracle at the bars of tests/test_gpu_loglike.py::test_no_step_count_flips_in_a_quarter_billion_solves."""
    from evidence_amd.layout import compile_layout
    from oracle.oracle import OracleModel
    w = make_workload(3)
    theta = w.sample_theta(20_000, seed=2024)
    got = ic.host_loglike(hi, w, theta)
    ref = OracleModel(compile_layout(w.parnames, w.fixedpardict, w.table.insts, []), w.table).loglike(theta, nthreads=8)
    err = golden.rel_err(got, ref)
    calm = theta[:, [w.parnames.index(f"planet{k}_ecc") for k in (1, 2, 3)]].max(axis=1) <= 0.95
    print(f"host log-L, 20000 cfg3 draws: p99.99 {np.percentile(err, 99.99):.2e}, calm max ({int(calm.sum())} rows) "
          f"{err[calm].max():.2e}, max {err.max():.2e}")
    assert np.percentile(err, 99.99) <= 1e-14
    assert calm.mean() > 0.97 and err[calm].max() <= 1e-13, float(err[calm].max())
    assert err.max() <= 1e-10, (float(err.max()), int(err.argmax()))
