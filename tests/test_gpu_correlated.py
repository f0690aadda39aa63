"""The correlated-noise likelihood on the device (rvll_celerite_loglike_batch, correlated.CorrelatedNoiseModel) against the dense
definition (correlated.log_likelihood_dense) applied to the model's own residuals, at the project's parity bound
|delta| <= 1e-10 max(1, |log-L|): every term kind, Q on both sides of and at the 1/2 clamp, every edge of the LDS epoch tile and
of the row blocks, a table that is not in time order with exact ties and a 3000-day gap; that a row's bits depend on the row
alone; the white limit; the flags and the refusals; and the evidence of a linear model in closed form.  Against the definition
in long double (correlated_cases.dense_reference), every row compared: every composition of columns with Q on a different side of
1/2 from lane to lane and invalid rows between them, log-uniform draws over a prior's decades on four tables, the band around
Q = 1/2 at sigma up to 100 svrad, and tables in time order (order = NULL), in decreasing time and with every epoch at one time.

Every agreement case prints its largest difference; profiles/celerite_probe.txt records the largest one seen."""
import os

import numpy as np
import pytest

import correlated_cases as cc
from evidence_amd import GpuRVModel, RvllError, _abi, correlated
from evidence_amd import priors as P
from evidence_amd.data import EpochTable
from evidence_amd.nested import run_nested_slice

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

B_FULL = 257                                 # five row blocks, the last with one row
B_CASES = (1, 63, 64, 65)
CHUNK_ROWS = 100                             # RVLL_CELERITE_CHUNK_ROWS: B_FULL then goes in three chunks
# every term of TERM_CASES under a prefix of its own, so that one model serves them all
ALL_TERMS = {"real": ("real", "gp1"), "sho": ("sho", "gp2"), "real2": ("real", "gp3"), "rotation": ("rotation", "gp4")}
RANGES = {"offset": (-3.0, 3.0), "jitter": (0.5, 2.0), "k1": (1.0, 6.0), "period": (3.0, 80.0), "ecc": (0.0, 0.5),
          "omega": (0.0, 2 * np.pi), "ma0": (0.0, 2 * np.pi), "lin": (-2.0, 2.0), "fwhm": (-0.5, 0.5)}
PLANET_NAMES = [f"planet{n}_{s}" for n in (1, 2) for s in ("k1", "period", "ecc", "omega", "ma0")]


def _noise_names():
    return [f"{prefix}_{s}" for kind, prefix in ALL_TERMS.values() for s in correlated.KINDS[kind][1]]


def _model(ne, planets, free_noise=True, fixed_noise=None, precision="fp64", priors=False):
    """The 0-planet model, or 2 planets with drift, a linear term and per-instrument jitter, on cc.make_table(ne)."""
    table = cc.make_table(ne)
    names, fixed, linpar = ["a_offset", "b_offset"], {}, None
    if planets:
        names += PLANET_NAMES + ["a_jitter", "b_jitter", "drift_lin", "linpar_fwhm"]
        fixed = {"planet1_epoch": 55000.0, "planet2_epoch": 55001.5}
        linpar = {"fwhm": np.random.default_rng(ne).normal(0.0, 1.0, ne)}
    if free_noise:
        names += _noise_names()
    if fixed_noise:
        fixed.update(fixed_noise)
    pri = None
    if priors:
        pri = {n: P.Uniform(*RANGES.get(n.split("_")[-1], (0.5, 30.0))) for n in names}
    return GpuRVModel(fixed, table, names, linpar_dict=linpar, priordict=pri, precision=precision)


def _theta(model, n, seed):
    rng = np.random.default_rng(seed)
    X = np.empty((n, model.ndim))
    for j, name in enumerate(model.parnames):
        lo, hi = RANGES.get(name.split("_")[-1], (1.0, 2.0))
        X[:, j] = rng.uniform(lo, hi, n)
    return X


def _set(model, X, values, jitter_seed=None):
    """Put a case's noise parameters into the rows of X; sigma, tau, rho and prot vary a little from row to row, q stays exact."""
    X = X.copy()
    rng = np.random.default_rng(jitter_seed)
    for name, v in values.items():
        col = np.full(X.shape[0], float(v))
        if jitter_seed is not None and name.split("_")[-1] in ("sigma", "tau", "rho", "prot"):
            col *= rng.uniform(0.9, 1.0, X.shape[0])
        X[:, model.parnames.index(name)] = col
    return X


def _rename(terms, values):
    """A case of cc.TERM_CASES under the prefixes of ALL_TERMS."""
    out_terms, out_values = [], {}
    for kind, prefix in terms:
        new = ALL_TERMS["real2" if kind == "real" and len(terms) > 1 else kind][1]
        out_terms.append((kind, new))
        for s in correlated.KINDS[kind][1]:
            out_values[f"{new}_{s}"] = values[f"{prefix}_{s}"]
    return out_terms, out_values


def _dense(gp, X, res, var, rows):
    return np.array([correlated.log_likelihood_dense(res[i], var[i], gp.table.time, gp.columns(X[i])) for i in rows])


@pytest.mark.parametrize("planets", [False, True], ids=["0planets", "2planets"])
@pytest.mark.parametrize("ne", cc.NE_CASES)
def test_device_matches_the_dense_definition_and_rows_are_independent(gpu_required, ne, planets):
    worst = 0.0
    with _model(ne, planets) as model:
        assert not np.array_equal(np.argsort(model.table.time, kind="stable"), np.arange(ne)) or ne < 3
        base = _theta(model, B_FULL, seed=ne)
        rows = list(range(66)) + [127, 128, 255, 256]                   # block edges and the last, one-row block
        for cid, terms, values in cc.TERM_CASES:
            terms, values = _rename(terms, values)
            gp = correlated.CorrelatedNoiseModel(model, terms)
            X = _set(model, base, values, jitter_seed=ne)
            res, var = model.residuals_batch(X)
            got, flags = gp.log_likelihood_batch(X, return_flags=True)
            assert not flags.any(), cid
            want = _dense(gp, X, res, var, rows)
            err = cc.rel_err(got[rows], want)
            print(f"ne {ne} planets {planets} {cid}: max rel err {err.max():.3e}")
            worst = max(worst, float(err.max()))
            assert err.max() <= cc.PARITY, (cid, err.max())
            # the same bits alone, in smaller batches, and across a chunk boundary
            for b in B_CASES:
                assert np.array_equal(gp.log_likelihood_batch(X[:b]), got[:b]), (cid, b)
            assert gp.log_likelihood(X[200]) == got[200]
            os.environ["RVLL_CELERITE_CHUNK_ROWS"] = str(CHUNK_ROWS)
            try:
                assert np.array_equal(gp.log_likelihood_batch(X), got), cid
                assert np.array_equal(gp.log_likelihood_batch(X[90:110]), got[90:110]), cid
            finally:
                del os.environ["RVLL_CELERITE_CHUNK_ROWS"]
    print(f"ne {ne} planets {planets}: largest rel err {worst:.3e}")


@pytest.mark.parametrize("planets", [False, True], ids=["0planets", "2planets"])
def test_fixed_noise_parameters_give_the_bits_of_free_ones(gpu_required, planets):
    ne = cc.EPOCH_BLOCK + 1
    values = {"gp1_sigma": 1.5, "gp1_tau": 40.0, "gp2_sigma": 2.5, "gp2_rho": 17.0, "gp2_q": 3.0, "gp3_sigma": 1.0, "gp3_tau": 5.0,
              "gp4_sigma": 2.0, "gp4_prot": 23.0, "gp4_q0": 0.8, "gp4_dq": 0.3, "gp4_mix": 0.7}
    cases = [[ALL_TERMS["real"]], [ALL_TERMS["sho"]], [ALL_TERMS["sho"], ALL_TERMS["real2"]], [ALL_TERMS["rotation"]]]
    with _model(ne, planets) as free, _model(ne, planets, free_noise=False, fixed_noise=values) as fixed:
        Xf = _set(free, _theta(free, 65, seed=3), values)
        Xx = np.ascontiguousarray(Xf[:, [free.parnames.index(n) for n in fixed.parnames]])
        for terms in cases:
            a = correlated.CorrelatedNoiseModel(free, terms).log_likelihood_batch(Xf)
            b = correlated.CorrelatedNoiseModel(fixed, terms).log_likelihood_batch(Xx)
            assert np.array_equal(a, b), terms
    # fixed wins over free
    with _model(ne, planets, free_noise=True, fixed_noise={"gp2_q": 3.0}) as both:
        X = _set(both, _theta(both, 5, seed=3), values)
        X[:, both.parnames.index("gp2_q")] = 0.2
        gp = correlated.CorrelatedNoiseModel(both, [ALL_TERMS["sho"]])
        res, var = both.residuals_batch(X)
        assert gp.columns(X[0])[0, 4] == correlated.FORM_COS
        assert cc.rel_err(gp.log_likelihood_batch(X), _dense(gp, X, res, var, range(5))).max() <= cc.PARITY


def test_prior_loglike_is_prior_then_loglike_bit_for_bit(gpu_required):
    with _model(cc.EPOCH_BLOCK + 1, True, priors=True) as model:
        gp = correlated.CorrelatedNoiseModel(model, [ALL_TERMS["sho"], ALL_TERMS["real2"]])
        cubes = np.random.default_rng(5).random((B_FULL, model.ndim))
        theta = gp.prior_transform_batch(cubes)
        assert np.array_equal(theta, model.prior_transform_batch(cubes))
        want, wflags = gp.log_likelihood_batch(theta, return_flags=True)
        th2, got, flags = gp.prior_loglike_batch(cubes, return_flags=True)
        assert np.array_equal(th2, theta) and np.array_equal(got, want) and np.array_equal(flags, wflags)
        assert (got > -1e29).all()
        os.environ["RVLL_CELERITE_CHUNK_ROWS"] = str(CHUNK_ROWS)
        try:
            th3, got3 = gp.prior_loglike_batch(cubes)
        finally:
            del os.environ["RVLL_CELERITE_CHUNK_ROWS"]
        assert np.array_equal(th3, theta) and np.array_equal(got3, want)
        assert np.array_equal(gp.prior_transform(cubes[3]), theta[3])


def test_white_limit(gpu_required):
    """sigma = 0: the white likelihood of the model itself, planets and jitter included."""
    for ne in (cc.EPOCH_BLOCK - 1, 2 * cc.EPOCH_BLOCK + 1):
        with _model(ne, True, free_noise=False, fixed_noise={"gp1_sigma": 0.0, "gp1_tau": 10.0}) as model:
            gp = correlated.CorrelatedNoiseModel(model, [("real", "gp1")])
            X = _theta(model, B_FULL, seed=9)
            got, flags = gp.log_likelihood_batch(X, return_flags=True)
            want = model.log_likelihood_batch(X)
            err = cc.rel_err(got, want)
            print(f"white limit ne {ne}: max rel err {err.max():.3e}")
            assert not flags.any() and err.max() <= cc.PARITY


def test_flags_and_refusals(gpu_required):
    ne = cc.EPOCH_BLOCK + 1
    table = cc.make_table(ne)
    names = ["a_offset", "b_offset", "planet1_k1", "planet1_period", "planet1_ecos", "planet1_esin", "planet1_ma0", "gp2_sigma",
             "gp2_rho", "gp2_q"]
    with GpuRVModel({"planet1_epoch": 55000.0}, table, names) as model:
        gp = correlated.CorrelatedNoiseModel(model, [("sho", "gp2")])
        X = _theta(model, 70, seed=2)
        ix = model.parnames.index
        X[:, ix("planet1_ecos")], X[:, ix("planet1_esin")] = 0.1, 0.2
        X[:, ix("gp2_sigma")], X[:, ix("gp2_rho")], X[:, ix("gp2_q")] = 2.0, 15.0, 1.5
        good = gp.log_likelihood_batch(X)
        bad = X.copy()
        bad[3, ix("planet1_ecos")], bad[3, ix("planet1_esin")] = 0.8, 0.8        # ecos^2 + esin^2 > 1
        bad[10, ix("gp2_rho")] = 0.0
        bad[64, ix("gp2_q")] = -1.0
        bad[65, ix("gp2_sigma")] = np.nan
        bad[66, ix("planet1_ecos")], bad[66, ix("planet1_esin")], bad[66, ix("gp2_q")] = 0.8, 0.8, -1.0   # the orbit's flag alone
        got, flags = gp.log_likelihood_batch(bad, return_flags=True)
        hit = [3, 10, 64, 65, 66]
        assert (got[hit] == -1e30).all()
        assert list(flags[hit]) == [_abi.FLAG_INVALID_ORBIT, _abi.FLAG_NOISE_INVALID, _abi.FLAG_NOISE_INVALID, _abi.FLAG_NOISE_INVALID,
                                    _abi.FLAG_INVALID_ORBIT]
        rest = np.setdiff1d(np.arange(70), hit)
        assert np.array_equal(got[rest], good[rest]) and not flags[rest].any()
        assert gp.columns(bad[10]) is None and gp.columns(bad[64]) is None and gp.columns(bad[65]) is None

        # a bad order
        order = gp.order.copy()
        for wrong in (order[::-1].copy(), np.zeros(ne, dtype=np.int32), np.arange(ne, dtype=np.int32), order + 1):
            gp.order = np.ascontiguousarray(wrong, dtype=np.int32)
            with pytest.raises(RvllError) as err:
                gp.log_likelihood_batch(X)
            assert err.value.code == _abi.E_INVALID
        ties = np.flatnonzero(np.diff(table.time[order]) == 0.0)
        assert ties.size > 0
        swapped = order.copy()
        swapped[[ties[0], ties[0] + 1]] = swapped[[ties[0] + 1, ties[0]]]           # ties may come in either order
        gp.order = swapped
        assert cc.rel_err(gp.log_likelihood_batch(X), good).max() <= cc.PARITY
        gp.order = order

        # the caps, an unknown kind, a slot outside theta
        lib, h = model._lib, model._h
        out, fl = np.empty(70), np.zeros(70, dtype=np.int32)

        def call(terms_c, n):
            return lib.rvll_celerite_loglike_batch(h, _abi.as_dp(X), 70, 0, terms_c, n, _abi.as_ip(order), None, _abi.as_dp(out),
                                                   _abi.as_ip(fl), None)
        five = (_abi.NoiseTerm * 5)()
        for t in five:
            t.kind = _abi.NOISE_REAL
            t.par[0], t.par[1] = _abi.Slot.fixed(1.0), _abi.Slot.fixed(5.0)
        assert call(five, 4) == _abi.OK and call(five, 5) == _abi.E_INVALID and call(five, 0) == _abi.E_INVALID
        five[0].kind = _abi.NOISE_SHO
        assert call(five, 3) == _abi.OK and call(five, 4) == _abi.E_INVALID                  # rank 5
        five[0].kind = 7
        assert call(five, 1) == _abi.E_INVALID
        five[0].kind = _abi.NOISE_REAL
        five[0].par[1] = _abi.Slot.free(model.ndim)
        assert call(five, 1) == _abi.E_INVALID
        five[0].par[1] = _abi.Slot.fixed(5.0)
        assert lib.rvll_celerite_loglike_batch(h, _abi.as_dp(X), -1, 0, five, 1, None, None, _abi.as_dp(out), _abi.as_ip(fl), None) == _abi.E_INVALID
        assert lib.rvll_celerite_loglike_batch(h, _abi.as_dp(X), 70, 0, five, 1, _abi.as_ip(order), None, None, _abi.as_ip(fl), None) == _abi.E_INVALID
        assert lib.rvll_celerite_loglike_batch(h, _abi.as_dp(X), 70, 1, five, 1, _abi.as_ip(order), None, _abi.as_dp(out), _abi.as_ip(fl),
                                               None) == _abi.E_NOPRIORS
        assert call(five, 1) == _abi.OK
    with _model(5, False, precision="fp32") as model32:
        gp = correlated.CorrelatedNoiseModel(model32, [ALL_TERMS["real"]])
        with pytest.raises(RvllError) as err:
            gp.log_likelihood_batch(_theta(model32, 4, seed=1))
        assert err.value.code == _abi.E_UNSUPPORTED


def test_callbacks_take_the_wrapper(gpu_required):
    from evidence_amd.callbacks import make_polychord_callbacks, make_ultranest_callbacks
    with _model(cc.EPOCH_BLOCK, False, priors=True) as model:
        gp = correlated.CorrelatedNoiseModel(model, [ALL_TERMS["sho"]])
        cubes = np.random.default_rng(1).random((9, gp.ndim))
        theta, want = gp.prior_loglike_batch(cubes)
        prior, loglike = make_ultranest_callbacks(gp, vectorized=True)
        assert np.array_equal(prior(cubes), theta) and np.array_equal(loglike(theta), want)
        prior1, loglike1, ndim, nderived = make_polychord_callbacks(gp)
        assert (ndim, nderived) == (gp.ndim, 0)
        assert np.array_equal(prior1(cubes[2]), theta[2]) and loglike1(theta[2]) == (want[2], [])


def _linear_case():
    """0 planets, 40 epochs, a fixed SHO term, free offset and linear drift under uniform priors 12 posterior sigma wide on each
    side of the generalised-least-squares solution: ln Z = log-L(beta) + 1/2 ln det(2 pi (A^T Sigma^-1 A)^-1) - ln(prior volume).
    -> (noise, table, priors, truth, (y, A, beta, svrad, t, cols))"""
    ne = 40
    rng = np.random.default_rng(40)
    t = 55000.0 + np.sort(rng.uniform(0.0, 120.0, ne))
    svrad = rng.uniform(0.8, 1.2, ne)
    noise = {"gp1_sigma": 2.0, "gp1_rho": 15.0, "gp1_q": 2.0}
    cols = correlated.term_columns("sho", [noise["gp1_sigma"], noise["gp1_rho"], noise["gp1_q"]])
    Sigma = np.diag(svrad ** 2) + correlated.kernel_matrix(t, cols)
    tt = (t - t[0]) / 365.25
    y = 1.0 + 6.0 * tt + np.linalg.cholesky(Sigma) @ rng.normal(size=ne)
    A = np.stack([np.ones(ne), tt], axis=1)
    Si = np.linalg.inv(Sigma)
    cov = np.linalg.inv(A.T @ Si @ A)
    beta = cov @ (A.T @ Si @ y)
    sd = np.sqrt(np.diag(cov))
    lo, hi = beta - 12.0 * sd, beta + 12.0 * sd
    truth = (correlated.log_likelihood_dense(y - A @ beta, svrad ** 2, t, cols) + 0.5 * np.log(np.linalg.det(2.0 * np.pi * cov))
             - np.log(np.prod(hi - lo)))
    table = EpochTable.from_arrays(["a"], t, y, svrad, np.zeros(ne, dtype=np.int32))
    pri = {"a_offset": P.Uniform(lo[0], hi[0]), "drift_lin": P.Uniform(lo[1], hi[1])}
    return noise, table, pri, truth, (y, A, beta, svrad, t, cols)


def test_evidence_of_a_linear_model_in_closed_form(gpu_required):
    noise, table, pri, truth, (y, A, beta, svrad, t, cols) = _linear_case()
    with GpuRVModel(noise, table, list(pri), priordict=pri) as model:
        gp = correlated.CorrelatedNoiseModel(model, [("sho", "gp1")])
        assert gp.parnames == ["a_offset", "drift_lin"]
        peak = gp.log_likelihood(beta)
        assert cc.rel_err(peak, correlated.log_likelihood_dense(y - A @ beta, svrad ** 2, t, cols)) <= cc.PARITY
        out = [run_nested_slice(gp.prior_transform_batch, gp.log_likelihood_batch, gp.ndim, nlive=400, dlogz=0.01, seed=s,
                                prior_loglike=gp.prior_loglike_batch) for s in (1, 2, 3)]
    for r in out:
        print(f"ln Z {r.logz:.4f} +- {r.logzerr:.4f}, truth {truth:.4f}")
    for r in out:
        assert abs(r.logz - truth) < 4 * r.logzerr + 0.05, (r.logz, r.logzerr, truth)


def test_evidence_of_a_linear_model_through_run_nested_ensemble(gpu_required):
    """The wrapper as a drop-in for run_nested_ensemble: its own slice_walk_runs walks under the correlated likelihood."""
    from evidence_amd.nested import run_nested_ensemble
    noise, table, pri, truth, _ = _linear_case()
    with GpuRVModel(noise, table, list(pri), priordict=pri) as model:
        gp = correlated.CorrelatedNoiseModel(model, [("sho", "gp1")])
        r, = run_nested_ensemble(gp.prior_transform_batch, gp.log_likelihood_batch, gp.ndim, [1], nlive=400, dlogz=0.01,
                                 walker_runs=gp.slice_walk_runs)
    print(f"ln Z {r.logz:.4f} +- {r.logzerr:.4f}, truth {truth:.4f}")
    assert abs(r.logz - truth) < 4 * r.logzerr + 0.05, (r.logz, r.logzerr, truth)


# ---- lane-mixed forms, the prior's range, the band at Q = 1/2 and the tables, against the long-double reference -----------------------
B_MIXED = 128                                # two waves of rows
NE_WIDE = 2 * cc.EPOCH_BLOCK + 1             # three epoch tiles, the last with one epoch
SUFFIXES = sorted({s for _, names in correlated.KINDS.values() for s in names})
WIDE_TABLES = {"ne65": lambda: cc.make_table(NE_WIDE), "ne64": lambda: cc.make_table(2 * cc.EPOCH_BLOCK),
               "ne96": lambda: cc.make_table(3 * cc.EPOCH_BLOCK), "cadence": cc.cadence_table, "sorted": cc.sorted_table,
               "decreasing": cc.decreasing_table, "ties": cc.ties_table}
ALONE = (0, 1, 2, 3, 4, 5, 6, 71)            # one row of every entry of cc.Q_SIDES and one of the second wave, none of them invalid


class _Models:
    """One model a (table, planets): every parameter of gp1 to gp4 free, so that one handle serves every composition."""

    def __init__(self):
        self.open = {}

    def get(self, table_id, planets):
        if (table_id, planets) not in self.open:
            table = WIDE_TABLES[table_id]()
            ne = table.time.size
            names, fixed, linpar = [f"{i}_offset" for i in table.insts], {}, None
            if planets:
                names += PLANET_NAMES + [f"{i}_jitter" for i in table.insts] + ["drift_lin", "linpar_fwhm"]
                fixed = {"planet1_epoch": 55000.0, "planet2_epoch": 55001.5}
                linpar = {"fwhm": np.random.default_rng(ne).normal(0.0, 1.0, ne)}
            names += [f"gp{k}_{s}" for k in (1, 2, 3, 4) for s in SUFFIXES]
            self.open[table_id, planets] = GpuRVModel(fixed, table, names, linpar_dict=linpar)
        return self.open[table_id, planets]

    def close(self):
        for m in self.open.values():
            m.close()


@pytest.fixture(scope="module")
def models():
    m = _Models()
    yield m
    m.close()


def _evaluate(model, terms, values, seed):
    """The rows of a generator on a model: X, the device's log-L and flags, the long-double reference on the model's own
    residuals (NaN where the definition has no covariance) and which rows are valid."""
    n = len(next(iter(values.values())))
    X = _theta(model, n, seed)
    for name, v in values.items():
        X[:, model.parnames.index(name)] = v
    gp = correlated.CorrelatedNoiseModel(model, terms)
    res, var = model.residuals_batch(X)
    cols, valid = cc.rows_columns(terms, values)
    assert np.array_equal(gp.columns(X[0]), cols[0])
    want = cc.dense_reference(res, var, model.table.time, cols)
    assert np.array_equal(np.isfinite(want), valid)
    got, flags = gp.log_likelihood_batch(X, return_flags=True)
    return gp, X, got, flags, want, valid


def _hold(label, got, flags, want, valid, bound=cc.PARITY):
    """Every row counts: the valid ones within the bound with no flag, the others refused."""
    err = cc.ref_err(got[valid], want[valid])
    print(f"{label}: max rel err {err.max():.3e} over {valid.sum()} rows against long double")
    assert err.max() <= bound, (label, int(np.flatnonzero(valid)[err.argmax()]), err.max())
    assert not flags[valid].any()
    assert (got[~valid] == -1e30).all() and (flags[~valid] == _abi.FLAG_NOISE_INVALID).all()
    return float(err.max())


@pytest.mark.parametrize("composition", list(cc.COMPOSITIONS))
def test_lane_mixed_forms(gpu_required, models, composition):
    """Neighbouring lanes run different forms (Q on every side of 1/2, invalid rows between them) in every composition."""
    for planets in (False, True):
        model = models.get("ne65", planets)
        terms, values = cc.mixed_rows(composition, B_MIXED, seed=2, svmin=model.table.svrad.min())
        gp, X, got, flags, want, valid = _evaluate(model, terms, values, seed=21)
        assert (~valid).sum() == B_MIXED // cc.INVALID_EVERY
        _hold(f"mixed {composition} planets {planets}", got, flags, want, valid)
        # a row alone gives the bits it had in the batch; so does the batch reversed, row by row
        for i in ALONE:
            assert valid[i] and gp.log_likelihood(X[i]) == got[i], (composition, i)
        back, bflags = gp.log_likelihood_batch(np.ascontiguousarray(X[::-1]), return_flags=True)
        assert np.array_equal(back[::-1], got) and np.array_equal(bflags[::-1], flags)
        # an invalid row leaves its neighbours alone: the batch with those rows repaired has the other rows' bits
        mended = X.copy()
        bad = np.flatnonzero(~valid)
        mended[bad] = X[bad - 1]
        again, aflags = gp.log_likelihood_batch(mended, return_flags=True)
        assert np.array_equal(again[valid], got[valid]) and np.array_equal(again[bad], got[bad - 1]) and not aflags.any()


@pytest.mark.parametrize("composition", ["2", "12", "22", "211", "rotation"])
@pytest.mark.parametrize("table_id", ["ne65", "ne64", "ne96", "cadence"])
def test_the_priors_range(gpu_required, models, table_id, composition):
    """Log-uniform draws over a prior's decades: d t up to 2e6 in the sincos, exp(-c dt) through underflow to 0, c of 1e5 a day,
    sigma up to 30 svrad."""
    for planets in (False, True):
        model = models.get(table_id, planets)
        terms, values = cc.wide_rows(composition, B_MIXED, seed=3, svmin=model.table.svrad.min())
        _, _, got, flags, want, valid = _evaluate(model, terms, values, seed=31)
        assert valid.all()
        _hold(f"wide {composition} {table_id} planets {planets}", got, flags, want, valid)


@pytest.mark.parametrize("composition", ["sho", "rotation"])
def test_the_band_around_q_one_half(gpu_required, models, composition):
    """sigma up to 100 svrad within 1e-4 of Q = 1/2 (cc.band_rows): the pair basis of csrc/rvll_celerite.h holds the bound where the
    two nearly cancelling columns lost 6.4e-9."""
    for planets in (False, True):
        model = models.get("ne65", planets)
        terms, values = cc.band_rows(model.table.svrad.min())[composition]
        _, _, got, flags, want, valid = _evaluate(model, terms, values, seed=41)
        assert valid.all()
        _hold(f"band {composition} planets {planets}", got, flags, want, valid)


def test_tables_in_time_order_decreasing_and_all_ties(gpu_required, models):
    # a table already in time order: order = NULL is the identity, bit for bit; NULL on a table that is not in order is refused
    model = models.get("sorted", True)
    terms, values = cc.mixed_rows("211", B_MIXED, seed=4, svmin=model.table.svrad.min())
    gp, X, got, flags, want, valid = _evaluate(model, terms, values, seed=51)
    assert np.array_equal(gp.order, np.arange(model.table.time.size))
    _hold("sorted 211", got, flags, want, valid)
    out, fl = np.empty(B_MIXED), np.zeros(B_MIXED, dtype=np.int32)

    def null_order(m, g, x):
        return m._lib.rvll_celerite_loglike_batch(m._h, _abi.as_dp(x), B_MIXED, 0, g._terms_c, len(g.terms), None, None, _abi.as_dp(out),
                                                  _abi.as_ip(fl), None)
    assert null_order(model, gp, X) == _abi.OK
    assert np.array_equal(out, got) and np.array_equal(fl, flags)
    unsorted = models.get("ne65", True)
    ugp = correlated.CorrelatedNoiseModel(unsorted, terms)
    assert null_order(unsorted, ugp, _theta(unsorted, B_MIXED, seed=52)) == _abi.E_INVALID
    # the same table listed in decreasing time
    model = models.get("decreasing", True)
    for which, composition in (("mixed", "22"), ("wide", "12")):
        terms, values = getattr(cc, which + "_rows")(composition, B_MIXED, seed=5, svmin=model.table.svrad.min())
        gp, X, got, flags, want, valid = _evaluate(model, terms, values, seed=53)
        assert np.array_equal(gp.order, np.arange(model.table.time.size)[::-1])
        _hold(f"decreasing {which} {composition}", got, flags, want, valid)
    # every epoch at one time: every gap is 0 and Sigma = diag(var) + sum(a) 1 1^T
    for planets in (False, True):
        model = models.get("ties", planets)
        for composition in ("1", "2", "rotation"):
            terms, values = cc.mixed_rows(composition, B_MIXED, seed=6, svmin=model.table.svrad.min())
            gp, X, got, flags, want, valid = _evaluate(model, terms, values, seed=54)
            _hold(f"ties {composition} planets {planets}", got, flags, want, valid)
            res, var = model.residuals_batch(X)
            i = int(np.flatnonzero(valid)[0])
            suma = sum(v[i] ** 2 for k, v in values.items() if k.endswith("_sigma"))
            S = np.diag(var[i]) + suma
            plain = -0.5 * res[i] @ np.linalg.solve(S, res[i]) - 0.5 * np.linalg.slogdet(S)[1] - 0.5 * res.shape[1] * np.log(2 * np.pi)
            assert cc.rel_err(got[i], plain) <= 1e-9             # (the columns' sum of a is sigma² to 1e-9 at the clamp)
