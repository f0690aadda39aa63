"""CPU: the correlated-noise likelihood's definitions (evidence_amd/correlated.py) — the recursion in numpy, and the kernel's own
source compiled for the host (csrc/rvll_celerite.h, tests/native/hostcelerite.hip), against the dense Cholesky definition at the
project's parity bound |delta| <= 1e-10 max(1, |log-L|); the kernel matrix; how names become slots; invalid parameters; the C
prototype.  Then the long-double reference of correlated_cases against mpmath, and both float64 implementations against it: within
a quarter of the bound where neighbouring rows differ in form and over a prior's range, and within the bound in the band around
Q = 1/2 at sigma up to 100 svrad."""
import ctypes as C

import numpy as np
import pytest

import correlated_cases as cc
from evidence_amd import _abi, correlated
from evidence_amd.layout import compile_layout

IDS = [c[0] for c in cc.TERM_CASES]


@pytest.fixture(scope="module")
def hc():
    lib = cc.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


def _row(ne, seed=0):
    table = cc.make_table(ne, seed)
    rng = np.random.default_rng(ne + 7)
    return table.time, rng.normal(0.0, 4.0, ne), table.svrad ** 2 + 0.25


@pytest.mark.parametrize("case", cc.TERM_CASES, ids=IDS)
@pytest.mark.parametrize("ne", cc.NE_CASES)
def test_the_recursion_matches_the_dense_definition(case, ne):
    _, terms, values = case
    t, res, var = _row(ne)
    cols = cc.case_columns(terms, values)
    want = correlated.log_likelihood_dense(res, var, t, cols)
    got = correlated.log_likelihood_recursive(res, var, t, cols)
    assert want > -1e29 and cc.rel_err(got, want) <= cc.PARITY, (got, want)


@pytest.mark.parametrize("case", cc.TERM_CASES, ids=IDS)
@pytest.mark.parametrize("ne", cc.NE_CASES)
def test_the_kernels_source_on_the_host_matches_the_dense_definition(hc, case, ne):
    _, terms, values = case
    t, res, var = _row(ne)
    want = correlated.log_likelihood_dense(res, var, t, cc.case_columns(terms, values))
    got, flag = cc.host_loglike(hc, terms, values, res, var, t)
    assert flag == 0 and cc.rel_err(got, want) <= cc.PARITY, (got, want)


@pytest.mark.parametrize("case", cc.TERM_CASES, ids=IDS)
def test_the_host_columns_are_the_definitions(hc, case):
    _, terms, values = case
    want = cc.case_columns(terms, values)
    j = 0
    for kind, prefix in terms:
        p = [values[f"{prefix}_{s}"] for s in correlated.KINDS[kind][1]]
        p = (C.c_double * 5)(*(p + [0.0] * (5 - len(p))))
        for sub in range(correlated.RANK[kind]):
            out = (C.c_double * 5)()
            assert hc.hc_column(correlated.KINDS[kind][0], sub, p, out) == 1
            np.testing.assert_allclose(list(out), want[j], rtol=1e-13, atol=0.0)
            j += 1
    assert j == want.shape[0]


@pytest.mark.parametrize("case", cc.TERM_CASES, ids=IDS)
def test_kernel_matrix_is_symmetric_with_the_sum_of_a_on_its_diagonal(case):
    _, terms, values = case
    t = cc.make_table(33).time
    cols = cc.case_columns(terms, values)
    K = correlated.kernel_matrix(t, cols)
    assert np.array_equal(K, K.T)
    suma = cols[cols[:, 4] != correlated.FORM_SIN, 0].sum()
    np.testing.assert_allclose(np.diag(K), suma, rtol=1e-14)
    sigma2 = sum(v * v for k, v in values.items() if k.endswith("_sigma"))
    np.testing.assert_allclose(suma, sigma2, rtol=1e-9)           # every kind's k(0) is sigma^2 (rtol: the 1 / f cancellation at the clamp)


def test_sho_is_continuous_across_q_one_half():
    t = cc.make_table(33).time
    K = [correlated.kernel_matrix(t, correlated.term_columns("sho", [3.0, 25.0, q])) for q in (0.5 - 1e-6, 0.5, 0.5 + 1e-6)]
    scale = np.abs(K[1]).max()
    assert np.abs(K[0] - K[2]).max() <= 1e-4 * scale and np.abs(K[1] - K[2]).max() <= 1e-4 * scale
    # inside the clamp q is taken at its edge, on the side it lies on; 1/2 itself counts as above
    assert correlated.term_columns("sho", [3.0, 25.0, 0.5]) == correlated.term_columns("sho", [3.0, 25.0, 0.5 + 1e-9])
    below = correlated.term_columns("sho", [3.0, 25.0, 0.5 - 1e-9])
    assert below[0][4] == correlated.FORM_REAL and below[0][2] == pytest.approx(correlated.term_columns("sho", [3.0, 25.0, 0.5 - 1e-6])[0][2], rel=1e-7)


def test_names_resolve_free_fixed_and_fixed_over_free():
    names = ["a_offset", "gp1_sigma", "gp1_rho", "gp1_q"]
    (kind, prefix, slots), = correlated.resolve_terms([("sho", "gp1")], names, {})
    order = sorted(names)
    assert (kind, prefix) == ("sho", "gp1")
    assert slots == [(order.index("gp1_sigma"), 0.0), (order.index("gp1_rho"), 0.0), (order.index("gp1_q"), 0.0)]
    (_, _, slots), = correlated.resolve_terms([("sho", "gp1")], ["a_offset", "gp1_sigma"], {"gp1_rho": 25, "gp1_q": 0.7})
    assert slots == [(1, 0.0), (-1, 25.0), (-1, 0.7)]
    (_, _, slots), = correlated.resolve_terms([("real", "gp7")], ["gp7_sigma", "gp7_tau"], {"gp7_tau": 9.0})      # fixed wins
    assert slots == [(0, 0.0), (-1, 9.0)]
    with pytest.raises(KeyError):
        correlated.resolve_terms([("sho", "gp1")], ["gp1_sigma", "gp1_rho"], {})
    for bad in ("gp", "gp1_", "planet1", "gpx", "1gp", "gp1 ", ""):
        with pytest.raises(ValueError):
            correlated.resolve_terms([("real", bad)], [f"{bad}_sigma", f"{bad}_tau"], {})
    with pytest.raises(ValueError):
        correlated.resolve_terms([("matern", "gp1")], [], {})
    fixed = {f"gp{i}_{s}": 1.0 for i in (1, 2, 3, 4, 5) for s in ("sigma", "tau", "rho", "q", "prot", "q0", "dq", "mix")}
    with pytest.raises(ValueError):                                # rank 5
        correlated.resolve_terms([("rotation", "gp1"), ("real", "gp2")], [], fixed)
    with pytest.raises(ValueError):
        correlated.resolve_terms([("sho", "gp1"), ("sho", "gp2"), ("real", "gp3")], [], fixed)
    with pytest.raises(ValueError):                                # five terms
        correlated.resolve_terms([("real", f"gp{i}") for i in (1, 2, 3, 4, 5)], [], fixed)
    with pytest.raises(ValueError):
        correlated.resolve_terms([], [], fixed)
    assert len(correlated.resolve_terms([("real", f"gp{i}") for i in (1, 2, 3, 4)], [], fixed)) == 4


def test_the_layout_ignores_the_noise_names():
    """A model built with the noise parameters among its names is the model without them, the indices aside."""
    base = ["a_offset", "a_jitter", "planet1_k1", "planet1_period", "planet1_ecc", "planet1_omega", "planet1_ma0", "drift_lin"]
    noise = ["gp1_sigma", "gp1_rho", "gp1_q", "gp2_sigma", "gp2_tau", "gp3_prot", "gp3_q0", "gp3_dq", "gp3_mix"]
    fixed = {"planet1_epoch": 55000.0}
    L0, L1 = compile_layout(base, fixed, ["a"]), compile_layout(base + noise, fixed, ["a"])
    assert L1.parnames == sorted(base + noise)
    assert (L1.nplanets, L1.has_jitter, L1.has_drift, L1.has_linpar) == (L0.nplanets, L0.has_jitter, L0.has_drift, L0.has_linpar) == (1, True, True, False)

    def named(L, slot):
        return L.parnames[slot.index] if slot.is_free else slot.value
    p0, p1 = L0.planets[0], L1.planets[0]
    for f in ("k", "p", "e1", "e2", "anom", "epoch"):
        assert named(L0, getattr(p0, f)) == named(L1, getattr(p1, f))
    assert named(L0, L0.insts[0].offset) == named(L1, L1.insts[0].offset) and named(L0, L0.insts[0].jitter) == named(L1, L1.insts[0].jitter)
    assert [named(L0, s) for s in L0.drift] == [named(L1, s) for s in L1.drift]
    from evidence_amd.callbacks import wrapped_params
    assert not wrapped_params(noise).any()


@pytest.mark.parametrize("kind, params", [
    ("real", [-1.0, 5.0]), ("real", [1.0, 0.0]), ("real", [np.nan, 5.0]), ("real", [1.0, np.inf]),
    ("sho", [1.0, 0.0, 1.0]), ("sho", [1.0, 5.0, -1.0]), ("sho", [1.0, 5.0, 0.0]), ("sho", [np.nan, 5.0, 1.0]), ("sho", [-0.1, 5.0, 1.0]),
    ("rotation", [1.0, 0.0, 1.0, 0.5, 0.5]), ("rotation", [1.0, 20.0, -0.5, 0.5, 0.5]), ("rotation", [1.0, 20.0, 1.0, 0.0, 0.5]),
    ("rotation", [1.0, 20.0, 1.0, 0.5, -0.1]), ("rotation", [1.0, 20.0, 1.0, 0.5, np.inf]),
])
def test_invalid_parameters_give_the_sentinel(hc, kind, params):
    assert correlated.term_columns(kind, params) is None
    t, res, var = _row(5)
    assert correlated.log_likelihood_dense(res, var, t, None) == -1e30
    assert correlated.log_likelihood_recursive(res, var, t, None) == -1e30
    values = {f"gp1_{s}": v for s, v in zip(correlated.KINDS[kind][1], params)}
    logl, flag = cc.host_loglike(hc, [(kind, "gp1")], values, res, var, t)
    assert logl == -1e30 and flag == _abi.FLAG_NOISE_INVALID


def test_a_matrix_that_is_not_positive_definite_and_a_nan_residual(hc):
    t, res, var = _row(5)
    cols = np.array([[-50.0, 0.0, 0.05, 0.0, 0.0]])                 # a negative real term larger than the white noise
    assert correlated.log_likelihood_dense(res, var, t, cols) == -1e30
    assert correlated.log_likelihood_recursive(res, var, t, cols) == -1e30
    # a rotation term whose second oscillator is not underdamped has no columns: NaN pivots refuse the row
    values = {"gp1_sigma": 1.0, "gp1_prot": 20.0, "gp1_q0": -0.25, "gp1_dq": 1.0, "gp1_mix": 0.5}
    assert correlated.log_likelihood_dense(res, var, t, cc.case_columns([("rotation", "gp1")], values)) == -1e30
    assert cc.host_loglike(hc, [("rotation", "gp1")], values, res, var, t) == (-1e30, _abi.FLAG_NOISE_INVALID)
    # an invalid orbit's NaN row: the orbit's flag alone, whatever the noise parameters are
    bad = res.copy()
    bad[2] = np.nan
    assert cc.host_loglike(hc, [("real", "gp1")], {"gp1_sigma": 1.0, "gp1_tau": 5.0}, bad, var, t) == (-1e30, _abi.FLAG_INVALID_ORBIT)
    assert cc.host_loglike(hc, [("real", "gp1")], {"gp1_sigma": -1.0, "gp1_tau": 5.0}, bad, var, t) == (-1e30, _abi.FLAG_INVALID_ORBIT)


def test_white_limit_of_the_definition():
    t, res, var = _row(33)
    want = -0.5 * np.sum(res ** 2 / var) - 0.5 * np.sum(np.log(var)) - 0.5 * 33 * np.log(2 * np.pi)
    for f in (correlated.log_likelihood_dense, correlated.log_likelihood_recursive):
        assert cc.rel_err(f(res, var, t, correlated.term_columns("real", [0.0, 10.0])), want) <= 1e-13


def test_the_prototype_and_the_abi_version():
    assert _abi.ABI_VERSION == (0, 8)
    restype, argtypes = _abi.PROTOTYPES["rvll_celerite_loglike_batch"]
    assert restype is C.c_int and len(argtypes) == 11
    assert argtypes[4] is C.POINTER(_abi.NoiseTerm) and C.sizeof(_abi.NoiseTerm) == 8 + 5 * 16
    assert hasattr(_abi.load(), "rvll_celerite_loglike_batch")
    assert (_abi.NOISE_REAL, _abi.NOISE_SHO, _abi.NOISE_ROTATION, _abi.FLAG_NOISE_INVALID) == (0, 1, 2, 8)
    assert (_abi.NOISE_MAX_TERMS, _abi.NOISE_MAX_RANK) == (4, 4)


# ---- the long-double reference, lane-mixed forms, the prior's range and the band at Q = 1/2 --------------------------------------------
NE_WIDE = 2 * cc.EPOCH_BLOCK + 1
N_ROWS = 64                                  # 63 consecutive rows hold every pair of Q sides of two SHOs (cc.Q_SIDES, Q_SIDES_2)


def _mp_loglike(res, var, t, cols):
    """log_likelihood_dense in mpmath at 50 digits, from the float64 inputs as they are."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    ne = len(t)
    tm = [mp.mpf(float(v)) for v in t]
    A = mp.matrix(ne, ne)
    for n in range(ne):
        for m in range(ne):
            x = abs(tm[n] - tm[m])
            k = mp.mpf(0)
            for a, b, c, d, form in cols:
                if int(form) != correlated.FORM_SIN:
                    k += mp.exp(-mp.mpf(float(c)) * x) * (mp.mpf(float(a)) * mp.cos(mp.mpf(float(d)) * x) + mp.mpf(float(b)) * mp.sin(mp.mpf(float(d)) * x))
            A[n, m] = k + (mp.mpf(float(var[n])) if n == m else 0)
    L = mp.cholesky(A)
    z = mp.lu_solve(L, mp.matrix([mp.mpf(float(v)) for v in res]))
    return -sum(v * v for v in z) / 2 - sum(mp.log(L[n, n]) for n in range(ne)) - ne * mp.log(2 * mp.pi) / 2


@pytest.mark.parametrize("kind, params", [
    ("real", [3.0, 20.0]), ("sho", [3.0, 25.0, 0.2]), ("sho", [3.0, 25.0, 4.0]), ("rotation", [3.0, 25.0, 1.0, 0.5, 0.5]),
    ("sho", [100.0, 25.0, 0.5 - 1e-6]), ("sho", [100.0, 25.0, 0.5 + 1e-6])],
    ids=["real", "sho_below", "sho_above", "rotation", "clamp_below_sigma100", "clamp_above_sigma100"])
def test_the_long_double_reference_against_mpmath(kind, params):
    mpmath = pytest.importorskip("mpmath")
    t, res, var = _row(12)
    cols = np.asarray(correlated.term_columns(kind, params))
    want = _mp_loglike(res, var, t, cols)
    got = cc.dense_reference(res, var, t, cols)
    got_mp = mpmath.mpf(np.format_float_scientific(got, precision=25, unique=False))        # 26 digits hold a long double
    err = abs(got_mp - want) / max(1, abs(want))
    print(f"{kind} {params}: long double against mpmath {float(err):.3e}")
    assert err <= 1e-16
    # the batched form gives the same bits a row as one row alone, and NaN where there is no covariance
    both = cc.dense_reference(np.stack([res, res, res]), np.stack([var, var, var]), t, np.stack([cols, np.full_like(cols, np.nan), cols]))
    assert both[0] == got and both[2] == got and np.isnan(both[1])


def test_the_long_double_reference_refuses_a_pivot_that_is_not_positive():
    t, res, var = _row(5)
    assert np.isnan(cc.dense_reference(res, var, t, np.array([[-50.0, 0.0, 0.05, 0.0, 0.0]])))
    bad = res.copy()
    bad[2] = np.nan
    assert np.isnan(cc.dense_reference(bad, var, t, np.asarray(correlated.term_columns("real", [1.0, 5.0]))))


_CASES = {}


def _case(which, composition):
    """The rows of a generator on cc.make_table(NE_WIDE) with N(0, 4) residuals and svrad in [1, 2], with their long-double
    reference, the numpy recursion and the host build: computed once, shared by the tests below."""
    key = (which, composition)
    if key not in _CASES:
        table = cc.make_table(NE_WIDE)
        t, var, svmin = table.time, table.svrad ** 2, table.svrad.min()
        if which == "band":
            terms, values = cc.band_rows(svmin)[composition]
        else:
            terms, values = getattr(cc, which + "_rows")(composition, N_ROWS, seed=1, svmin=svmin)
        cols, valid = cc.rows_columns(terms, values)
        n = len(valid)
        res = np.random.default_rng([n, NE_WIDE]).normal(0.0, 4.0, (n, NE_WIDE))
        want = cc.dense_reference(res, np.broadcast_to(var, res.shape), t, cols)
        rec = np.array([correlated.log_likelihood_recursive(res[i], var, t, cols[i] if valid[i] else None) for i in range(n)])
        lib = cc.host_lib()
        host = None if lib is None else np.array([cc.host_loglike(lib, terms, cc.row_values(values, i), res[i], var, t) for i in range(n)])
        _CASES[key] = (valid, want, rec, host)
    return _CASES[key]


def _check(which, composition, bound):
    valid, want, rec, host = _case(which, composition)
    assert np.array_equal(np.isfinite(want), valid)              # the reference has a value exactly where the definition has columns
    assert valid.sum() >= len(valid) - len(valid) // cc.INVALID_EVERY - 1
    err = cc.ref_err(rec[valid], want[valid])
    print(f"{which} {composition}: the numpy recursion against long double {err.max():.3e}")
    assert err.max() <= bound, (which, composition, np.flatnonzero(valid)[err.argmax()], err.max())
    assert (rec[~valid] == -1e30).all()
    assert host is not None, "hipcc was not found: the host build of the kernel's source is half of this test"
    err = cc.ref_err(host[valid, 0], want[valid])
    print(f"{which} {composition}: the kernel's source on the host against long double {err.max():.3e}")
    assert err.max() <= bound, (which, composition, np.flatnonzero(valid)[err.argmax()], err.max())
    # the flag is FLAG_NOISE_INVALID exactly where term_columns gives None or NaN columns
    assert (host[valid, 1] == 0).all() and (host[~valid, 1] == _abi.FLAG_NOISE_INVALID).all() and (host[~valid, 0] == -1e30).all()


@pytest.mark.parametrize("composition", list(cc.COMPOSITIONS))
def test_lane_mixed_forms_stay_within_a_quarter_of_the_bound(composition):
    """Every ordered composition of real and SHO columns with Q on every side of 1/2 from row to row and every 13th row invalid:
    both float64 implementations within PARITY / 4 of the long-double reference, which is what lets the GPU tests ask PARITY."""
    valid, _, _, _ = _case("mixed", composition)
    assert (~valid).sum() == N_ROWS // cc.INVALID_EVERY
    _check("mixed", composition, cc.PARITY / 4)


@pytest.mark.parametrize("composition", list(cc.COMPOSITIONS))
def test_the_priors_range_stays_within_a_quarter_of_the_bound(composition):
    """Timescales from 0.01 to 1e4 days across a 3000-day gap, Q from 0.01 to 1e4, sigma up to 30 svrad."""
    valid, _, _, _ = _case("wide", composition)
    assert valid.all()
    _check("wide", composition, cc.PARITY / 4)


@pytest.mark.parametrize("composition", ["sho", "rotation"])
def test_the_band_around_q_one_half_meets_the_bound(composition):
    """sigma up to 100 svrad at |Q - 1/2| <= 1e-4, where the two columns of an SHO nearly cancel: without the pair basis of
    csrc/rvll_celerite.h (cel_prepare) the recursion is off by 6.4e-9 at sigma = 100 svrad, 2.3e-11 (sigma / 3 svrad)² in general."""
    valid, _, _, _ = _case("band", composition)
    assert valid.all()
    _check("band", composition, cc.PARITY)


def test_the_generators_cover_what_they_claim():
    assert sorted(cc.COMPOSITIONS) == sorted(["1", "2", "11", "12", "21", "111", "22", "112", "121", "211", "1111", "rotation"])
    for cid, kinds in cc.COMPOSITIONS.items():
        assert sum(correlated.RANK[k] for k in kinds) <= _abi.NOISE_MAX_RANK
        assert [p for _, p in cc.composition_terms(cid)] == [f"gp{k + 1}" for k in range(len(kinds))]
    # 64 consecutive rows of two SHOs hold every pair of sides, and neighbouring rows differ
    terms, values = cc.mixed_rows("22", 128, seed=1)
    cols, valid = cc.rows_columns(terms, values)

    def side(q):
        return [i for i, s in enumerate(cc.Q_SIDES) if s == q] or [0 if q < 0.5 else 6]
    for start in (0, 64):
        seen = set()
        for i in range(start, start + 64):
            if valid[i]:
                seen.add((side(values["gp1_q"][i])[0], side(values["gp2_q"][i])[0]))
        assert len(seen) >= 45                                   # 49 pairs, less those the invalid rows took
        forms = {(cols[i, 0, 4], cols[i, 2, 4]) for i in range(start, start + 64) if valid[i]}
        assert forms == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}
    assert (np.diff(values["gp1_q"]) != 0).all()
    # the invalid rows rotate through every fault
    for cid in cc.COMPOSITIONS:
        terms, values = cc.mixed_rows(cid, 128, seed=1)
        _, valid = cc.rows_columns(terms, values)
        assert list(np.flatnonzero(~valid)) == list(range(cc.INVALID_EVERY - 1, 128, cc.INVALID_EVERY))
        terms, values = cc.wide_rows(cid, 128, seed=1, svmin=1.0)
        total = np.sqrt(sum(v ** 2 for k, v in values.items() if k.endswith("_sigma")))
        assert total.max() <= 30.0 * (1 + 1e-12) and all((np.abs(v - 0.5) >= 1e-3).all() for k, v in values.items() if k.endswith("_q"))
    band = cc.band_rows(1.0)
    assert band["sho"][1]["gp1_q"].size == len(cc.BAND_RATIOS) * len(cc.BAND_DQ) * len(cc.BAND_RHO)
    # the tables
    for table in (cc.sorted_table(), cc.cadence_table()):
        assert np.array_equal(np.argsort(table.time, kind="stable"), np.arange(table.time.size)) and (np.diff(table.time) > 0).all()
    assert np.array_equal(cc.decreasing_table().time, cc.sorted_table().time[::-1])
    assert np.ptp(cc.ties_table().time) == 0.0 and cc.ties_table().time.size == 5
    assert np.diff(cc.cadence_table().time).max() < 4e-4
