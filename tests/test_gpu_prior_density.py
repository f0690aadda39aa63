"""Prior densities on the device (rvll_prior_logpdf_batch; sensitivity.log_prior_sets / GpuRVModel.log_prior_batch with a
device) against the numpy definition (priors.log_density) and the reference's golden values, both at the project's parity bound
|delta| <= 1e-10 max(1, |value|) with -inf and NaN in the same places; the same bits in any batching; malformed input is
refused by the entry; and the density against the transform the sampler applies.

Shapes: the rows around one workgroup (64 rows: 1, 63, 64, 65), several workgroups with a tail (257, 1000); one, several and
more parameters than a set chunk has sets; 1, 3 and 130 sets (130 = 8 chunks of 16 sets and a tail of 2).

Transform against density.  q = linspace(0.001, 0.999, 65) goes through rvll_prior_batch, exp(logpdf) from the device is
integrated between consecutive theta with Simpson's rule on 65 points, and the result is compared with q[i + 1] - q[i] = 0.998 /
64 (the steps of that grid; 1 / 64 would be those of linspace(0, 1, 65)).  The bound of a case is 4 times what the same check
gives for the reference's own `.ppf` / `.pdf` pair on the CPU (tests/golden/gen_prior_density_golden.py measures it into
prior_density.json: the device inverts its tables in its own arithmetic).  Measured for the reference, largest per family:
    Uniform 1.6e-16   Jeffreys 1.7e-13   ModJeffreys 1.7e-14   TruncatedRayleigh 4.2e-11   Normal 1.9e-11   LogNormal 3.1e-8
    Gamma 2.2e-10   Beta 2.8e-8   Alpha 6.5e-6 (Simpson's own error at the steep start of the density)
    table kinds: Binormal 1.0e-7   AsymmetricNormal 1.6e-7   TruncatedUNormal 2.4e-8   PowerLaw 1.5e-7   Sine 3.5e-9
                 DoublePowerLaw 1.0e-5 (the kink at x0 inside a Simpson step)
UniformFrequency and Log10Normal have no such pair in the reference (its UniformFrequency `.pdf` has no support, its
Log10Normal `.ppf` raises): their bound is 4 times the largest of the table kinds, 4.2e-5.  A density wrong by 1 % misses a step
by 1.6e-4, above every bound.  Measured on the MI355X: the reference's figure to three digits in every case (Jeffreys(10, 100)
3.1e-16 against 3.0e-16); UniformFrequency(1, 100) 8.1e-10, UniformFrequency(0.05, 500) 4.6e-6, Log10Normal 7.6e-8."""
import ctypes as C

import numpy as np
import pytest

import prior_density_cases as dc
from evidence_amd import GpuRVModel, _abi, priors as P, sensitivity
from evidence_amd.synthetic import make_workload
from test_gpu_priors import one_param_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

CASES = dc.golden_cases()
TABLE_KINDS = ("Binormal", "AsymmetricNormal", "TruncatedUNormal", "PowerLaw", "DoublePowerLaw", "Sine")
UNPAIRED_BOUND = 4.0 * max(c[4] for c in CASES if c[0] in TABLE_KINDS)
CONSISTENCY = [(c[0], c[1], 4.0 * c[4]) for c in CASES] + [("UniformFrequency", (1.0, 100.0), UNPAIRED_BOUND),
                                                          ("UniformFrequency", (0.05, 500.0), UNPAIRED_BOUND),
                                                          ("Log10Normal", (0.5, 0.7), UNPAIRED_BOUND),
                                                          ("Log10Normal", (-1.0, 0.2), UNPAIRED_BOUND)]


@pytest.mark.parametrize("n_sets", [1, 3, 130])
@pytest.mark.parametrize("ndim", [1, 7, 12])
def test_the_device_matches_the_definition(gpu_required, ndim, n_sets):
    sets = dc.mixed_sets(n_sets, ndim)
    worst, finite = 0.0, 0
    for B in (1, 63, 64, 65, 257, 1000):
        th = dc.rows(B, ndim, seed=B + ndim)
        timing = {}
        got = sensitivity.log_prior_sets(sets, th, device=0, timing=timing)
        want = sensitivity.log_prior_sets(sets, th)
        worst = max(worst, dc.assert_parity(got, want, (B, ndim, n_sets)))
        finite += int(np.isfinite(want).sum())
        assert timing["rows"] == B and timing["elements"] == B * n_sets * ndim and timing["launches"] == 1 and timing["threads"] == 64
    assert finite > 0
    print(f"ndim {ndim}, {n_sets} sets: largest error over max(1, |value|) {worst:.2e}; {finite} finite values")


def test_every_kind_is_in_the_mixed_sets():
    kinds = {s.density[0] for specs in dc.mixed_sets(130, 12) for s in specs if s is not None}
    assert kinds == set(range(1, 20)) and any(s is None for specs in dc.mixed_sets(3, 7) for s in specs)


def test_the_device_matches_the_reference(gpu_required):
    worst = {}
    for case in CASES:
        name, args, x, want, _ = case
        got = sensitivity.log_prior_sets([[P.distdict[name](*args)]], x[:, None], device=0)[:, 0]
        worst[dc.case_id(case)] = dc.assert_parity(got, want, dc.case_id(case))
    print("largest error over max(1, |value|):", max(worst, key=worst.get), max(worst.values()))


def test_bits_are_the_same_in_any_batching(gpu_required):
    sets = dc.mixed_sets(130, 12)
    th = dc.rows(1000, 12, seed=4)
    whole = sensitivity.log_prior_sets(sets, th, device=0)
    parts = np.concatenate([sensitivity.log_prior_sets(sets, th[a:b], device=0) for a, b in ((0, 1), (1, 64), (64, 1000))])
    assert np.array_equal(whole.view(np.uint64), parts.view(np.uint64))
    again = sensitivity.log_prior_sets(sets, th, device=0)
    assert np.array_equal(whole.view(np.uint64), again.view(np.uint64))
    # a set's column does not depend on the sets next to it
    alone = sensitivity.log_prior_sets(sets[17:18], th, device=0)
    assert np.array_equal(whole[:, 17].view(np.uint64), alone[:, 0].view(np.uint64))


def test_the_models_log_prior_is_the_stateless_entry(gpu_required):
    w = make_workload(3)                                                 # 19 parameters, a Beta prior among them
    pri = w.priordict()
    with GpuRVModel(w.fixedpardict, w.table, w.parnames, priordict=pri, device=0) as model:
        theta = model.prior_transform_batch(w.sample_cube(300, seed=3))
        got = model.log_prior_batch(theta)
        outside = theta[:5].copy()
        outside[:, w.parnames.index("planet1_ecc")] = 1.5
        assert np.all(np.isneginf(model.log_prior_batch(outside)))
    sets = [[pri[name] for name in w.parnames]]
    assert got.shape == (300,) and np.all(np.isfinite(got))
    assert np.array_equal(got, sensitivity.log_prior_sets(sets, theta, device=0)[:, 0])
    dc.assert_parity(got, P.log_density(sets[0], theta))


def _raw(sets, ndim, theta, B, out="ok", n_sets=None, null=None):
    arr = (_abi.PriorDensity * max(1, len(sets)))()
    for i, (kind, group, args) in enumerate(sets):
        arr[i].kind, arr[i].group = kind, group
        for k, v in enumerate(args):
            arr[i].args[k] = v
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    res = np.zeros(max(1, theta.shape[0]) * max(1, len(sets)))
    n_sets = len(sets) // max(ndim, 1) if n_sets is None else n_sets
    return _abi.load().rvll_prior_logpdf_batch(0, None if null == "sets" else arr, n_sets, ndim, None if null == "theta" else _abi.as_dp(theta),
                                               B, None if null == "out" else _abi.as_dp(res), None)


GOOD = [(_abi.DENSITY_UNIFORM, -1, (0.0, 1.0)), (_abi.DENSITY_NORMAL, -1, (0.0, 1.0))]


@pytest.mark.parametrize("kw", [
    dict(null="sets"), dict(null="theta"), dict(null="out"), dict(B=0), dict(B=-1), dict(B=2 ** 30), dict(ndim=0), dict(ndim=65),
    dict(n_sets=0), dict(n_sets=4097),
    dict(sets=[(20, -1, (0.0, 1.0)), GOOD[1]]), dict(sets=[(-1, -1, (0.0, 1.0)), GOOD[1]]),
    dict(sets=[(_abi.DENSITY_UNIFORM, -1, (1.0, 1.0)), GOOD[1]]), dict(sets=[GOOD[0], (_abi.DENSITY_NORMAL, -1, (0.0, -1.0))]),
    dict(sets=[(_abi.DENSITY_JEFFREYS, -1, (0.0, 10.0)), GOOD[1]]), dict(sets=[(_abi.DENSITY_BETA, -1, (2.0, 0.0, 0.0)), GOOD[1]]),
    dict(sets=[(_abi.DENSITY_POWERLAW, -1, (-1.0, 1.0, 2.0, 0.0)), GOOD[1]]),
    dict(sets=[(_abi.DENSITY_UNIFORM, -1, (float("nan"), 1.0)), GOOD[1]]),
    dict(sets=[(_abi.DENSITY_SORTED_UNIFORM, 0, (0.0, 1.0)), (_abi.DENSITY_SORTED_LOGUNIFORM, 0, (0.5, 1.0))]),
    dict(sets=[(_abi.DENSITY_SORTED_UNIFORM, -1, (0.0, 1.0)), GOOD[1]]),
], ids=lambda kw: ",".join(f"{k}={v if not isinstance(v, list) else v[0][0]}" for k, v in kw.items()))
def test_malformed_input_is_refused_by_the_entry(gpu_required, kw):
    kw = dict(kw)
    sets, ndim = kw.pop("sets", GOOD), kw.pop("ndim", 2)
    theta = np.full((4, 2), 0.5)
    rc = _raw(sets, ndim, theta, kw.pop("B", 4), **kw)
    assert rc == _abi.E_INVALID
    assert len(_abi.load().rvll_last_error()) > 0
    assert _raw(GOOD, 2, theta, 4) == _abi.OK


def _simpson_steps(theta, logpdf):
    """The integral of exp(logpdf) between consecutive theta, Simpson's rule on 65 points each."""
    x = np.linspace(theta[:-1], theta[1:], 65, axis=1)
    f = np.exp(logpdf(x.reshape(-1))).reshape(x.shape)
    h = (theta[1:] - theta[:-1]) / 64.0
    return h / 3.0 * (f[:, 0] + 4.0 * f[:, 1:-1:2].sum(axis=1) + 2.0 * f[:, 2:-1:2].sum(axis=1) + f[:, -1])


@pytest.mark.parametrize("name,args,bound", CONSISTENCY, ids=[f"{n}{tuple(a)}" for n, a, _ in CONSISTENCY])
def test_the_density_is_that_of_the_transform(gpu_required, name, args, bound):
    spec = P.distdict[name](*args)
    q = np.linspace(0.001, 0.999, 65)
    with one_param_model(spec) as m:
        theta = m.prior_transform_batch(q.reshape(-1, 1))[:, 0]
    assert np.all(np.diff(theta) > 0)
    steps = _simpson_steps(theta, lambda x: sensitivity.log_prior_sets([[spec]], x[:, None], device=0)[:, 0])
    err = float(np.max(np.abs(steps - np.diff(q))))
    print(f"{name}{tuple(args)}: largest |integral - step| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, args, err, bound)
