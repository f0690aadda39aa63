"""CPU: the correlated-noise likelihood's definitions (evidence_amd/correlated.py) — the recursion in numpy, and the kernel's own
source compiled for the host (csrc/rvll_celerite.h, tests/native/hostcelerite.hip), against the dense Cholesky definition at the
project's parity bound |delta| <= 1e-10 max(1, |log-L|); the kernel matrix; how names become slots; invalid parameters; the C
prototype."""
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
