"""CPU: the prior densities (evidence_amd/priors.py: log_density, the numpy definition; csrc/rvll_prior_density.h compiled for
the host, tests/native/hostdensity.hip) against the reference's `.logpdf` golden values (tests/golden/prior_density.npz) at the
project's parity bound |delta| <= 1e-10 max(1, |value|), -inf exactly; the two kinds whose density is not the reference's
`.pdf` by their own statements; the joint density of the sorted kinds; the C prototype and struct."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import prior_density_cases as dc
from evidence_amd import _abi, priors as P

CASES = dc.golden_cases()


@pytest.fixture(scope="module")
def hd():
    lib = dc.host_lib()
    if lib is None:
        pytest.skip("hipcc not available")
    return lib


@pytest.mark.parametrize("case", CASES, ids=[dc.case_id(c) for c in CASES])
def test_the_numpy_definition_matches_the_reference(case):
    name, args, x, want, _ = case
    spec = P.distdict[name](*args)
    got = P.log_density([spec], x[:, None])
    dc.assert_parity(got, want, dc.case_id(case))
    assert np.isnan(P.log_density([spec], [[np.nan]])[0])
    lo, hi = P.support(spec)
    inside = np.isfinite(want)
    assert np.all((x[inside] >= lo) & (x[inside] <= hi)) and np.all((x[~inside] <= lo) | (x[~inside] >= hi))


@pytest.mark.parametrize("case", CASES, ids=[dc.case_id(c) for c in CASES])
def test_the_host_build_of_the_header_matches_the_reference(hd, case):
    name, args, x, want, _ = case
    spec = P.distdict[name](*args)
    dc.assert_parity(dc.host_logpdf(hd, spec, x), want, dc.case_id(case))
    assert np.isnan(dc.host_logpdf(hd, spec, [np.nan])[0])


def test_every_family_of_distdict_is_covered_or_pinned_here():
    covered = {c[0] for c in CASES}
    assert covered | {"UniformFrequency", "Log10Normal", "SortedUniform", "SortedLogUniform"} == set(P.distdict)
    assert all(sum(1 for c in CASES if c[0] == name) >= 2 for name in covered)
    example = dict(Uniform=(0, 1), Jeffreys=(1, 2), ModJeffreys=(1, 2), UniformFrequency=(1, 2), Normal=(0, 1), LogNormal=(1, 0, 1),
                   Log10Normal=(0, 1), Binormal=(0, 1, 1, 1, 0), AsymmetricNormal=(0, 1, 2), TruncatedUNormal=(0, 1, -1, 1),
                   TruncatedRayleigh=(1, 2), PowerLaw=(1, 0, 1), DoublePowerLaw=(1, -2, 1, 0.5, 2), Sine=(0, 90), Alpha=(1,), Beta=(1, 1),
                   Gamma=(1, 1), SortedUniform=(0, 1), SortedLogUniform=(1, 2))
    for name, factory in P.distdict.items():
        spec = factory(*example[name])
        assert spec.density is not None and 0 < spec.density[0] < 20 and len(spec.density) - 1 <= _abi.DENSITY_NARGS, name


@pytest.mark.parametrize("args", [(1.0, 100.0), (0.05, 500.0)])
def test_uniform_frequency_is_the_reference_inside_and_cut_outside(hd, args):
    """The reference's `_pdf` (xmax xmin) / (x^2 (xmax - xmin)) has no support cut; the transform only reaches [xmin, xmax]."""
    xmin, xmax = args
    x = np.concatenate([np.linspace(xmin, xmax, 201), [xmin * 0.999, xmin - 1.0, -xmin, xmax * 1.001, xmax * 30.0]])
    with np.errstate(all="ignore"):
        want = np.log((xmax * xmin) / (x ** 2 * (xmax - xmin)))
    want[201:] = -np.inf
    spec = P.UniformFrequency(*args)
    for got in (P.log_density([spec], x[:, None]), dc.host_logpdf(hd, spec, x)):
        dc.assert_parity(got, want)


@pytest.mark.parametrize("args", [(0.5, 0.7), (-1.0, 0.2)])
def test_log10normal_is_the_reference_minus_its_jacobian(hd, args):
    """The reference's `_pdf` is stats.norm.pdf(log10 x, mu, sigma) with the Jacobian 1 / (x ln 10) commented out."""
    from scipy import stats
    mu, sigma = args
    x = np.concatenate([10.0 ** np.linspace(mu - 6 * sigma, mu + 6 * sigma, 201), [0.0, -1.0, -1e300]])
    with np.errstate(all="ignore"):
        want = stats.norm.logpdf(np.log10(x), mu, sigma) - np.log(x * np.log(10.0))
    want[201:] = -np.inf
    spec = P.Log10Normal(*args)
    for got in (P.log_density([spec], x[:, None]), dc.host_logpdf(hd, spec, x)):
        dc.assert_parity(got, want)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["SortedUniform", "SortedLogUniform"])
def test_sorted_kinds_credit_the_joint_density_once_and_refuse_a_broken_order(name, n):
    a, b = (2.0, 7.0) if name == "SortedUniform" else (0.5, 40.0)
    spec = P.distdict[name](a, b)
    other = P.Normal(0.0, 1.0)
    dims = [0, 2, 3][:n]                                                 # members apart from each other, others between
    specs = [other] * 5
    for d in dims:
        specs[d] = spec
    rng = np.random.default_rng(n)
    th = rng.normal(0.0, 1.0, (200, 5))
    th[:, dims] = np.sort(rng.uniform(a, b, (200, n)), axis=1)
    rest = P.log_density([other if s is other else None for s in specs], th)
    const = math.lgamma(n + 1.0) - n * (math.log(b - a) if name == "SortedUniform" else math.log(math.log(b / a)))
    want = rest + const - (np.log(th[:, dims]).sum(axis=1) if name == "SortedLogUniform" else 0.0)
    got = P.log_density(specs, th)
    assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want)))
    terms = P.log_density_terms(specs, th)
    if name == "SortedUniform":
        assert np.all(terms[:, dims[:-1]] == 0.0) and np.all(terms[:, dims[-1]] == const)
    for i, j in itertools.combinations(range(n), 2):                     # any transposition of two different values
        swapped = th.copy()
        swapped[:, [dims[i], dims[j]]] = swapped[:, [dims[j], dims[i]]]
        assert np.all(np.isneginf(P.log_density(specs, swapped)))
    for d, v in ((dims[0], a - 1e-9), (dims[-1], b + 1e-9)):             # below a, above b
        out = th.copy()
        out[:, d] = v
        assert np.all(np.isneginf(P.log_density(specs, out)))
    ends = th[:1].copy()
    ends[0, dims] = np.linspace(a, b, n) if n > 1 else a                 # the closed ends
    assert np.isfinite(P.log_density(specs, ends)[0])
    nan = th[:1].copy()
    nan[0, dims[0]] = np.nan
    assert np.isnan(P.log_density(specs, nan)[0])


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_host_build_of_the_sorted_density_is_the_definition(hd, n):
    for name, (a, b), kind in (("SortedUniform", (2.0, 7.0), _abi.DENSITY_SORTED_UNIFORM),
                               ("SortedLogUniform", (0.5, 40.0), _abi.DENSITY_SORTED_LOGUNIFORM)):
        specs = [P.distdict[name](a, b)] * n
        rng = np.random.default_rng(10 + n)
        th = rng.uniform(a - 0.5, b + 0.5, (500, n))
        th[::2] = np.sort(th[::2], axis=1)
        th[5, 0] = np.nan
        want = P.log_density_terms(specs, th)
        for d in range(n):
            prev = np.ascontiguousarray(th[:, max(d - 1, 0)])
            x = np.ascontiguousarray(th[:, d])
            got = np.empty(500)
            last = d == n - 1
            hd.hd_sorted(C.c_int(kind), C.c_double(a), C.c_double(b), C.c_int(n if last else 0),
                         C.c_double(math.lgamma(n + 1.0) if last else 0.0), C.c_int(1 if d == 0 else 0), prev.ctypes.data_as(dc.dp),
                         x.ctypes.data_as(dc.dp), C.c_long(500), got.ctypes.data_as(dc.dp))
            dc.assert_parity(got, want[:, d], (name, n, d))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_sorted_uniform_density_integrates_to_one_over_the_cube(n):
    """exp of the SortedUniform(0, 1) joint density, n! on the ordered simplex and 0 elsewhere, summed over the midpoints of an
    m^n grid of the unit cube: the cells off the diagonal are counted exactly, the m^(n - 1) (n = 2: m; n = 3: 3 m^2 - 2 m)
    cells with two equal midpoints count whole (ties are in order) where half of each belongs, so the sum is above 1 by
    at most n! * (cells with a tie) / (2 m^n) — the grid's own error."""
    m = 60
    mid = (np.arange(m) + 0.5) / m
    grid = np.stack(np.meshgrid(*([mid] * n), indexing="ij"), axis=-1).reshape(-1, n)
    dens = np.exp(P.log_density([P.SortedUniform(0.0, 1.0)] * n, grid))
    total = dens.sum() / m ** n
    ties = {1: 0, 2: m, 3: 3 * m * m - 2 * m}[n]
    assert 1.0 - 1e-12 <= total <= 1.0 + math.factorial(n) * ties / (2.0 * m ** n) + 1e-12, total


def test_a_partly_listed_or_mixed_sorted_group_is_what_the_members_say():
    """Two groups of one kind are apart by their group id; one group of two kinds is refused."""
    a, b = P.SortedUniform(0.0, 1.0), P.SortedUniform(0.0, 1.0)
    b.group = 7
    th = np.array([[0.9, 0.1]])
    assert np.isneginf(P.log_density([a, a], th)[0]) and P.log_density([a, b], th)[0] == 0.0
    mixed = P.SortedLogUniform(0.5, 2.0)
    mixed.group = 0
    with pytest.raises(P.PriorError):
        P.log_density([a, mixed], th)


def test_abi_of_the_density_entry():
    assert "rvll_prior_logpdf_batch" in _abi.PROTOTYPES
    assert _abi.ABI_VERSION == (0, 8)
    assert C.sizeof(_abi.PriorDensity) == 8 + 8 * 8 and _abi.DENSITY_NARGS == 8
    assert _abi.DENSITY_SKIP == 0
    c = P.density_to_c(P.Beta(0.867, 3.03))
    assert c.kind == _abi.DENSITY_BETA and list(c.args)[:2] == [0.867, 3.03] and c.args[3] == 0.0
    skip = P.density_to_c(None)
    assert skip.kind == _abi.DENSITY_SKIP
    header = (dc.HERE.parent / "include" / "rvll.h").read_text()
    for name in dir(_abi):
        if name.startswith("DENSITY_") and name != "DENSITY_NARGS":
            assert f"RVLL_{name} = {getattr(_abi, name)}," in header, name


def test_the_header_refuses_what_the_factories_refuse(hd):
    bad = [(_abi.DENSITY_UNIFORM, (1.0, 1.0)), (_abi.DENSITY_JEFFREYS, (0.0, 1.0)), (_abi.DENSITY_MODJEFFREYS, (2.0, 1.0)),
           (_abi.DENSITY_UNIFORMFREQUENCY, (-1.0, 1.0)), (_abi.DENSITY_NORMAL, (0.0, 0.0)), (_abi.DENSITY_LOGNORMAL, (0.0, 0.0, 1.0)),
           (_abi.DENSITY_LOG10NORMAL, (0.0, -1.0)), (_abi.DENSITY_TRUNCRAYLEIGH, (0.0, 1.0)),
           (_abi.DENSITY_TRUNCUNORMAL, (0.0, 0.0, 0.0, 1.0, 0.0)), (_abi.DENSITY_POWERLAW, (-1.0, 1.0, 2.0, 0.0)),
           (_abi.DENSITY_DOUBLEPOWERLAW, (-1.0, -2.0, 1.0, 0.5, 2.0, 0.0)), (_abi.DENSITY_SINE, (90.0, 10.0, 0.0)),
           (_abi.DENSITY_BINORMAL, (1.0, 1.0, 0.0, 1.0, 0.0)), (_abi.DENSITY_ASYMNORMAL, (0.0, 1.0, 0.0)), (_abi.DENSITY_ALPHA, (0.0, 0.5)),
           (_abi.DENSITY_BETA, (0.0, 1.0, 0.0)), (_abi.DENSITY_GAMMA, (1.0, 0.0, 0.0)), (_abi.DENSITY_SORTED_UNIFORM, (1.0, 0.0)),
           (_abi.DENSITY_SORTED_LOGUNIFORM, (0.0, 1.0)), (_abi.DENSITY_UNIFORM, (np.nan, 1.0)), (20, (0.0, 1.0)), (-1, (0.0, 1.0))]
    for kind, args in bad:
        a = (C.c_double * _abi.DENSITY_NARGS)(*args)
        assert hd.hd_args_ok(C.c_int(kind), a) == 0, (kind, args)
    for spec in dc.CATALOGUE:
        a = (C.c_double * _abi.DENSITY_NARGS)(*spec.density[1:])
        assert hd.hd_args_ok(C.c_int(spec.density[0]), a) == 1, spec.name
