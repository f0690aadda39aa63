"""CPU: prior sensitivity of ln Z from merged runs (evidence_amd/sensitivity.py), the numpy definitions throughout.  Four small
synthetic runs, built as the pointwise host tests build theirs, with samples drawn for their rows: the identity alternative, the
half-width uniform (ln 2 in every replicate), the reweighted evidence against logsumexp(logwt + ln r) on the weights
merge.replicates_arrays returns, refused alternatives, and p(k | y) over the models."""
import math

import numpy as np
import pytest
from scipy.special import logsumexp

from evidence_amd import fip, merge, pointwise, priors as P, sensitivity
from evidence_amd.nested import NestedResult
from test_merge_host import _arrays, _synthetic

PARNAMES = ["a_k1", "b_period", "c_offset"]
BASE = {"a_k1": P.Uniform(0.0, 20.0), "b_period": P.Jeffreys(1.0, 1000.0), "c_offset": P.Normal(0.0, 10.0)}
LPD_BOUND = 2.5e-10                                # the pointwise tests' own bound on lpd


def _runs(seed=0):
    rng = np.random.default_rng(seed)
    return [_synthetic(rng, 12, 60, kbatch=3, tie_grid=0.5), _synthetic(rng, 30, 300, kbatch=10, off=5, tie_grid=0.5),
            _synthetic(rng, 8, 24, kbatch=2, off=3), _synthetic(rng, 20, 200)]


def _samples(n, seed=0):
    """Rows the base priors can have drawn: k1 below 10 in every row."""
    rng = np.random.default_rng(100 + seed)
    return np.stack([rng.uniform(0.1, 9.9, n), np.exp(rng.uniform(0.0, math.log(1000.0), n)), rng.normal(0.0, 4.0, n)], axis=1)


def _results(seed=0):
    out = []
    for i, (logl, birth) in enumerate(_runs(seed)):
        out.append(NestedResult(logz=0.0, logzerr=0.0, niter=0, ncall=0, information=0.0, samples=_samples(logl.size, 10 * seed + i),
                                logl=logl, logwt=np.zeros_like(logl), logl_birth=birth))
    return out


def test_the_identity_alternative_changes_nothing():
    res = _results()
    out = sensitivity.prior_sensitivity(res, PARNAMES, BASE, [dict(BASE), {"a_k1": P.Uniform(0.0, 20.0)}, {}], nsamples=8, seed=3)
    assert np.all(out["logratio"] == 0.0)
    assert np.all(np.abs(out["replicates"]["dlogz"]) <= 1e-14) and np.all(np.abs(out["dlogz"]) <= 1e-14)
    assert np.all(np.abs(out["replicates"]["efficiency"] - 1.0) <= 1e-14) and np.all(np.abs(out["efficiency"] - 1.0) <= 1e-14)
    assert np.all(out["outside"] == 0) and np.all(out["dlogz_err"] <= 1e-14)
    logz, info = merge.replicates(res, 8, seed=3)
    assert np.array_equal(out["replicates"]["logz"], logz) and np.array_equal(out["replicates"]["information"], info)
    assert out["logz_base"] == merge.merge(res).logz
    assert np.all(np.abs(out["logz"] - out["logz_base"]) <= 1e-14 * abs(out["logz_base"]))


@pytest.mark.parametrize("mode,bootstrap", [("random", True), ("expected", False)])
def test_half_the_width_of_a_uniform_prior_is_ln_2_in_every_replicate(mode, bootstrap):
    """Every k1 is below 10, so r = 2 on every row and sum p r / P = 2 whatever the weights."""
    out = sensitivity.prior_sensitivity(_results(), PARNAMES, BASE, [{"a_k1": P.Uniform(0.0, 10.0)}], nsamples=9, seed=1, mode=mode,
                                        bootstrap=bootstrap)
    assert np.all(np.abs(out["replicates"]["dlogz"] - math.log(2.0)) <= 1e-12)
    assert abs(out["dlogz"][0] - math.log(2.0)) <= 1e-12 and out["dlogz_err"][0] <= 1e-12
    assert np.all(np.abs(out["replicates"]["efficiency"] - 1.0) <= 1e-12) and out["outside"][0] == 0
    assert np.all(np.abs(out["replicates"]["logz_new"] - (out["replicates"]["logz"][:, None] + math.log(2.0))) <= 1e-12)


@pytest.mark.parametrize("mode,bootstrap", [("random", True), ("random", False), ("expected", True)])
def test_dlogz_is_the_logsumexp_of_the_reweighted_rows(mode, bootstrap):
    res = _results(1)
    alts = [{"a_k1": P.Uniform(0.0, 5.0)},                                        # excludes rows with weight
            {"b_period": P.UniformFrequency(1.0, 1000.0)},                          # another family on the same support
            {"c_offset": P.Normal(1.0, 3.0), "a_k1": P.ModJeffreys(1.0, 20.0)},     # two parameters at once
            {"b_period": P.Jeffreys(2.0, 500.0), "c_offset": P.TruncatedUNormal(0.0, 10.0, -30.0, 30.0)}]
    out = sensitivity.prior_sensitivity(res, PARNAMES, BASE, alts, nsamples=7, seed=11, mode=mode, bootstrap=bootstrap)
    samples, logl, birth, run_start = pointwise._samples(res)
    logz, info, logwt = merge.replicates_arrays(logl, birth, run_start, 7, seed=11, mode=mode, bootstrap=bootstrap, return_logwt=True)
    order = merge.merge_arrays(logl, birth, run_start)["order"]
    lr = out["logratio"][order]
    with np.errstate(invalid="ignore"):
        want = np.stack([logsumexp(logwt + lr[:, a][None, :], axis=1) for a in range(len(alts))], axis=1)
        kish = np.stack([2.0 * logsumexp(logwt + lr[:, a][None, :], axis=1) - logsumexp(logwt + 2.0 * lr[:, a][None, :], axis=1)
                         for a in range(len(alts))], axis=1)
    live = np.isfinite(logz)
    assert live.any()
    assert np.all(np.abs(out["replicates"]["dlogz"][live] - want[live]) <= LPD_BOUND)
    assert np.all(np.abs(np.log(out["replicates"]["efficiency"][live]) - kish[live]) <= 2 * LPD_BOUND)
    assert np.all(out["replicates"]["efficiency"][live] <= 1.0 + 1e-12) and np.all(out["replicates"]["efficiency"][live] > 0.0)
    assert np.array_equal(out["replicates"]["logz"], logz, equal_nan=True)
    # by hand: the ratio of the first alternative is 4 below 5 and 0 above; the last cuts the periods; the others leave no row out
    k1, per = samples[:, 0], samples[:, 1]
    assert np.array_equal(np.isneginf(out["logratio"][:, 0]), k1 > 5.0) and np.all(np.isfinite(out["logratio"][:, 1:3]))
    assert np.array_equal(np.isneginf(out["logratio"][:, 3]), (per < 2.0) | (per > 500.0))
    assert np.all(np.abs(out["logratio"][k1 <= 5.0, 0] - math.log(4.0)) <= 1e-14)
    m = merge.merge_arrays(logl, birth, run_start)
    weighted = m["order"][m["logwt"] >= pointwise.WEIGHT_FLOOR]
    assert out["outside"][0] == np.count_nonzero(k1[weighted] > 5.0) > 0 and np.all(out["outside"][1:3] == 0)
    assert out["outside"][3] == np.count_nonzero((per[weighted] < 2.0) | (per[weighted] > 500.0))
    assert np.all(np.isfinite(out["dlogz"])) and np.all(out["dlogz_min"] <= out["dlogz_max"])


def test_an_alternative_that_leaves_no_row_with_weight_has_no_evidence():
    res = _results()
    with np.errstate(invalid="ignore"):
        out = sensitivity.prior_sensitivity(res, PARNAMES, BASE, [{"a_k1": P.Uniform(12.0, 20.0)}, {"a_k1": P.Uniform(0.0, 10.0)}],
                                            nsamples=5, seed=2)
    assert np.all(np.isneginf(out["replicates"]["dlogz"][:, 0])) and np.all(np.isneginf(out["replicates"]["logz_new"][:, 0]))
    assert np.isneginf(out["dlogz"][0]) and np.isneginf(out["logz"][0]) and out["efficiency"][0] == 0.0
    assert out["outside"][0] > 0 and np.all(np.isneginf(out["logratio"][:, 0]))
    assert abs(out["dlogz"][1] - math.log(2.0)) <= 1e-12                 # the alternative next to it is not touched


def test_log_prior_sets_is_log_density_over_the_listed_parameters():
    th = _samples(50)
    sets = [[BASE[p] for p in PARNAMES], [None, BASE["b_period"], None], [None, None, None]]
    got = sensitivity.log_prior_sets(sets, th)
    assert got.shape == (50, 3) and np.all(got[:, 2] == 0.0)
    assert np.array_equal(got[:, 0], P.log_density(sets[0], th))
    assert np.all(np.abs(got[:, 1] + np.log(th[:, 1]) + math.log(math.log(1000.0))) <= 1e-13)
    with pytest.raises(ValueError):
        sensitivity.log_prior_sets([[None, None]], th)


def test_alternatives_outside_the_base_prior_are_refused():
    res = _results()
    for alt in ({"a_k1": P.Uniform(0.0, 30.0)}, {"a_k1": P.Uniform(-1.0, 10.0)}, {"b_period": P.Jeffreys(0.5, 10.0)},
                {"a_k1": P.Normal(5.0, 1.0)}, {"b_period": P.LogNormal(1.0, 0.0, 10.0)}):
        with pytest.raises(ValueError, match="support"):
            sensitivity.prior_sensitivity(res, PARNAMES, BASE, [alt], nsamples=2)
    with pytest.raises(ValueError, match="not a free parameter"):
        sensitivity.prior_sensitivity(res, PARNAMES, BASE, [{"planet9_k1": P.Uniform(0.0, 1.0)}], nsamples=2)
    # a real line is inside a real line, a half line inside a half line
    sensitivity.alternative_sets(PARNAMES, BASE, [{"c_offset": P.Binormal(0.0, 1.0, 5.0, 2.0, 0.3)}])
    sensitivity.alternative_sets(["x"], {"x": P.Gamma(2.0, 3.0)}, [{"x": P.LogNormal(0.5, 0.0, 2.0)}, {"x": P.Beta(2.0, 5.0)}])


def test_a_sorted_group_is_overridden_whole_or_not_at_all():
    names = ["p1", "p2", "q"]
    base = {"p1": P.SortedUniform(0.0, 10.0), "p2": P.SortedUniform(0.0, 10.0), "q": P.Uniform(0.0, 1.0)}
    with pytest.raises(ValueError, match="in part"):
        sensitivity.alternative_sets(names, base, [{"p1": P.SortedUniform(0.0, 5.0)}])
    with pytest.raises(ValueError, match="sorted"):
        sensitivity.alternative_sets(names, base, [{"p1": P.Uniform(0.0, 5.0), "p2": P.Uniform(0.0, 5.0)}])
    bsets, asets = sensitivity.alternative_sets(names, base, [{"p1": P.SortedUniform(0.0, 5.0), "p2": P.SortedUniform(0.0, 5.0)}])
    th = np.array([[1.0, 2.0, 0.5], [1.0, 7.0, 0.5]])
    ratio = sensitivity.log_prior_sets(asets, th) - sensitivity.log_prior_sets(bsets, th)
    assert abs(ratio[0, 0] - 2.0 * math.log(2.0)) <= 1e-14 and np.isneginf(ratio[1, 0])
    # a sorted alternative inside an unsorted base is fine: the ordered part of the box
    sensitivity.alternative_sets(["u", "v"], {"u": P.Uniform(0.0, 1.0), "v": P.Uniform(0.0, 1.0)},
                                 [{"u": P.SortedUniform(0.0, 1.0), "v": P.SortedUniform(0.0, 1.0)}])


def test_malformed_ratios_are_refused():
    logl, birth, run_start = _arrays(_runs())
    for bad in (np.full((logl.size, 1), np.nan), np.full((logl.size, 1), np.inf), np.zeros((logl.size - 1, 1)),
                np.full((logl.size, 1), 1e29)):
        with pytest.raises(ValueError):
            sensitivity.reweight_arrays(bad, logl, birth, run_start, nsamples=2)


def test_model_probabilities_sum_to_one_and_are_fips_for_the_identity():
    names = [["c_offset"], ["a_k1", "b_period", "c_offset"]]
    pri = [{"c_offset": BASE["c_offset"]}, BASE]
    res = []
    for k in range(2):
        runs = _results(2 + k)
        if k == 0:
            for r in runs:
                r.samples = r.samples[:, 2:]
        res.append(runs)
    alts = [{}, {"a_k1": P.Uniform(0.0, 10.0)}, {"b_period": P.UniformFrequency(1.0, 1000.0), "c_offset": P.Normal(0.0, 5.0)}]
    sens = sensitivity.sensitivity_per_model(res, names, pri, alts, seed=5, nsamples=6)
    out = sensitivity.model_probabilities(sens)
    assert out["pky"].shape == (2, 3) and out["pky_replicates"].shape == (6, 2, 3)
    assert np.all(np.abs(out["pky"].sum(axis=0) - 1.0) <= 1e-14) and np.all(np.abs(out["pky_replicates"].sum(axis=1) - 1.0) <= 1e-14)
    base_logz = [merge.merge(r).logz for r in res]
    assert np.all(np.abs(out["pky"][:, 0] - fip.model_probabilities([base_logz])) <= 1e-14)
    for k in range(2):                                                   # model k's replicates are those of its own seed
        logz, _ = merge.replicates(res[k], 6, seed=fip.model_seed(5, k))
        assert np.array_equal(sens[k]["replicates"]["logz"], logz)
    rep = np.stack([s["replicates"]["logz"] for s in sens], axis=1)
    assert np.all(np.abs(out["pky_replicates"][:, :, 0] - fip._softmax(rep)) <= 1e-14)
    assert np.all(np.abs(out["pky_err"] - np.std(out["pky_replicates"], axis=0)) == 0.0)
    # k1 applies to the one-planet model alone: its evidence doubles, the other's stays
    assert np.all(np.abs(sens[0]["replicates"]["dlogz"][:, 1]) <= 1e-14)
    assert np.all(np.abs(sens[1]["replicates"]["dlogz"][:, 1] - math.log(2.0)) <= 1e-12)
    odds = out["pky"][1] / out["pky"][0]
    assert abs(odds[1] / odds[0] - 2.0) <= 1e-11
    with pytest.raises(ValueError):
        sensitivity.model_probabilities([sens[0], dict(sens[1], replicates=dict(logz_new=np.zeros((5, 3))))])
