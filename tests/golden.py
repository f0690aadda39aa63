"""Loaders for the committed golden fixtures (tests/golden/*.npz, made by gen_golden.py
from the reference itself)."""
import hashlib
import json
from pathlib import Path

import numpy as np

from evidence_amd.data import EpochTable
from evidence_amd.layout import compile_layout

GOLDEN = Path(__file__).resolve().parent / "golden"


class Case:
    def __init__(self, name, table, parnames, fixed, theta, logL, linpar=None, note=""):
        self.name, self.table, self.parnames, self.fixed = name, table, list(parnames), dict(fixed)
        self.theta, self.logL, self.linpar, self.note = theta, logL, linpar or {}, note
        self.layout = compile_layout(self.parnames, self.fixed, table.insts, list(self.linpar))

    @property
    def linpar_series(self):
        if not self.layout.linpar_names:
            return None
        return np.stack([self.linpar[k] for k in self.layout.linpar_names])

    def __repr__(self):
        return f"Case({self.name})"


def _table(z, prefix, insts):
    return EpochTable.from_arrays(insts, z[f"{prefix}time"], z[f"{prefix}vrad"], z[f"{prefix}svrad"],
                                  z[f"{prefix}inst_id"])


def config_case(cfg):
    z = np.load(GOLDEN / f"loglike_cfg{cfg}.npz")
    insts = [str(s) for s in z["insts"]]
    fixed = {str(k): float(v) for k, v in zip(z["fixed_names"], z["fixed_values"])}
    return Case(f"cfg{cfg}", _table(z, "", insts), [str(s) for s in z["parnames"]], fixed, z["theta"], z["logL"])


def edge_cases():
    z = np.load(GOLDEN / "loglike_edges.npz")
    meta = json.loads((GOLDEN / "loglike_edges.json").read_text())
    inst_names = {"t1": ["ia"], "t2": ["ia", "ib"], "t3": ["ia", "ib", "ic"]}
    out = []
    for i, m in enumerate(meta):
        table = _table(z, f"{m['table']}_", inst_names[m["table"]])
        linpar = {k: z[f"c{i}_linpar_{k}"] for k in m["linpar"]}
        # gen_golden passed linpar as a dict in insertion order rhk, fwhm; the reference iterates that dict
        if linpar:
            linpar = {k: linpar[k] for k in ("rhk", "fwhm") if k in linpar}
        out.append(Case(m["name"], table, m["parnames"], m["fixed"], z[f"c{i}_theta"], z[f"c{i}_logL"], linpar,
                        m.get("note", "")))
    return out


def peg51_cases():
    z = np.load(GOLDEN / "loglike_51peg.npz")
    meta = json.loads((GOLDEN / "loglike_51peg.json").read_text())
    table = _table(z, "", ["hamilton"])
    return [Case(f"51peg_{m['name']}", table, m["parnames"], m["fixed"], z[f"{m['name']}_theta"],
                 z[f"{m['name']}_logL"]) for m in meta]


def high_ecc_case():
    """Eccentricity sweep 0.90 .. 0.9925 of one planet (gen_golden.py, gen_high_ecc): the solver's sensitive corner."""
    z = np.load(GOLDEN / "loglike_high_ecc.npz")
    insts = [str(s) for s in z["insts"]]
    fixed = {str(k): float(v) for k, v in zip(z["fixed_names"], z["fixed_values"])}
    return Case("high_ecc_sweep", _table(z, "", insts), [str(s) for s in z["parnames"]], fixed, z["theta"], z["logL"])


def wild_case():
    """Adversarial parameter ranges (gen_golden.py, gen_wild)."""
    z = np.load(GOLDEN / "loglike_wild.npz")
    insts = [str(s) for s in z["insts"]]
    fixed = {str(k): float(v) for k, v in zip(z["fixed_names"], z["fixed_values"])}
    return Case("wild_sweep", _table(z, "", insts), [str(s) for s in z["parnames"]], fixed, z["theta"], z["logL"])


def all_loglike_cases():
    return [config_case(c) for c in (1, 2, 3, 4, 5)] + edge_cases() + peg51_cases() + [high_ecc_case(), wild_case()]


class CurveCase:
    """One case of keprv_edges.npz: the edge case itself, the leading rows of its theta, the times and the reference's curves
    {"exNone", "ex1", .., "pl1", ..} [rows, len(times)]; an orbit for which the reference returns None is a NaN row."""

    def __init__(self, case, theta, times, curves, far):
        self.case, self.name, self.theta, self.times, self.curves, self.far = case, case.name, theta, times, curves, far
        self.nplanets = case.layout.nplanets

    def __repr__(self):
        return f"CurveCase({self.name})"


def keprv_edge_cases():
    """The curves of every edge case with a planet (gen_golden.py, gen_keprv_edges)."""
    z = np.load(GOLDEN / "keprv_edges.npz")
    meta = json.loads((GOLDEN / "keprv_edges.json").read_text())
    cases = {c.name: c for c in edge_cases()}
    out = []
    for m in meta:
        name = m["name"]
        assert cases[name].layout.nplanets == m["nplanets"]
        out.append(CurveCase(cases[name], z[f"{name}_theta"], z[f"{name}_times"], {k: z[f"{name}_{k}"] for k in m["keys"]},
                             m["far"]))
    return out


def residual_edge_cases():
    """[(case, z)] of residuals_edges.npz (gen_residuals_golden.py, gen_edges): z holds {name}_theta, _res, _var, _kep
    [3, Ne] and, for more than one planet, {name}_pl{p}, the reference's modelk of planet p at the epochs."""
    z = np.load(GOLDEN / "residuals_edges.npz")
    return [(c, z) for c in edge_cases() + [high_ecc_case(), wild_case()]]


def curve_mask(nplanets, key):
    """The include mask (bit p - 1: planet p) of a curve key of keprv.npz / keprv_edges.npz."""
    if key.startswith("pl"):
        return 1 << (int(key[2:]) - 1)
    mask = (1 << nplanets) - 1
    return mask if key == "exNone" else mask & ~(1 << (int(key[2:]) - 1))


def decode_planets(case, theta):
    """K, P, ecc, omega, ma0, epoch [rows, nplanets] and valid [rows] of theta by the lines of the reference's modelk
    (rvmodel:411-459), from the parameter names."""
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    n, npl = theta.shape[0], case.layout.nplanets

    def par(name):
        if name in case.parnames:
            return theta[:, case.parnames.index(name)]
        return np.full(n, case.fixed[name]) if name in case.fixed else None

    out = {k: np.zeros((n, npl)) for k in ("K", "P", "ecc", "omega", "ma0", "epoch")}
    valid = np.ones(n, dtype=bool)
    for i in range(npl):
        p = f"planet{i + 1}_"
        K, P = par(p + "k1"), par(p + "period")
        out["K"][:, i] = K if K is not None else np.exp(par(p + "logk1"))
        out["P"][:, i] = P if P is not None else np.exp(par(p + "logperiod"))
        if par(p + "secos") is not None:
            a, b = par(p + "secos"), par(p + "sesin")
            ecc, omega = a ** 2 + b ** 2, np.arctan2(b, a)
            valid &= ~(ecc > 1)
        elif par(p + "ecos") is not None:
            a, b = par(p + "ecos"), par(p + "esin")
            ecc, omega = np.sqrt(a ** 2 + b ** 2), np.arctan2(b, a)
            valid &= ~(ecc > 1)
        else:
            ecc, omega = par(p + "ecc"), par(p + "omega")
        ml0 = par(p + "ml0")
        out["ma0"][:, i] = ml0 - omega if ml0 is not None else par(p + "ma0")
        out["ecc"][:, i], out["omega"][:, i], out["epoch"][:, i] = ecc, omega, par(p + "epoch")
    out["valid"] = valid
    return out


WANDERING_CURVE_CASES = ("ecc_0p98", "ecc_clamp_below_0p989", "ecc_above_clamp_0p995")


def curve_bound(case, theta, times, ref, mask):
    """[rows, 1]: how far a curve may lie from the reference's `ref` [rows, len(times)].  1e-11 of max(1, the row's amplitude),
    the bar of tests/test_gpu_curves.py, plus what one unit in the last place of P, of the epoch or of 2 pi / P — which another
    exp may give — moves the curve by: 4 * 2^-52 * max |M| in the mean anomaly, carried through d nu / d M <= sqrt(1 - e^2) /
    (1 - e)^2 with e = min(ecc, 0.99), the solver's clamp, and |d rv / d nu| <= K, over the planets of `mask`."""
    d = decode_planets(case, theta)
    with np.errstate(invalid="ignore"):
        amp = np.nan_to_num(np.nanmax(np.abs(ref), axis=1, initial=0.0))
    ec = np.minimum(d["ecc"], 0.99)
    M = 2 * np.pi / d["P"][:, :, None] * (np.asarray(times)[None, None, :] - d["epoch"][:, :, None]) + d["ma0"][:, :, None]
    gain = np.abs(d["K"]) * np.sqrt(1 - ec ** 2) / (1 - ec) ** 2
    use = np.array([(mask >> i) & 1 for i in range(d["K"].shape[1])], dtype=float)
    slack = 4 * 2.0 ** -52 * np.abs(M).max(axis=(1, 2)) * (gain * use[None, :]).sum(axis=1)
    return (1e-11 * np.maximum(1.0, amp) + np.where(d["valid"], slack, 0.0))[:, None]


def check_curves(cc, key, got):
    """`got` against the reference's curves `key` of the CurveCase cc: NaN rows exactly where the reference returned None, every
    other element within curve_bound — or, for the three cases whose solves wander so that their stop may land a step apart, within
    the allowance of test_curves_on_the_eccentricity_sweep: 5e-9 of the amplitude, at most 0.1 % of the elements beyond 1e-10 of
    it.  Returns the largest |got - ref| over its bound."""
    ref = cc.curves[key]
    assert got.shape == ref.shape, (cc.name, key)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (cc.name, key)
    ok = ~np.isnan(ref).any(axis=1)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - ref[ok])
    if cc.name in WANDERING_CURVE_CASES:
        d = err / np.maximum(1.0, np.abs(ref[ok]).max(axis=1, keepdims=True))
        assert d.max() <= 5e-9, (cc.name, key, float(d.max()))
        assert (d > 1e-10).mean() <= 0.001, (cc.name, key, float((d > 1e-10).mean()))
        return float(d.max() / 5e-9)
    ratio = err / curve_bound(cc.case, cc.theta, cc.times, ref, curve_mask(cc.nplanets, key))[ok]
    assert ratio.max() <= 1.0, (cc.name, key, float(ratio.max()), int(ratio.argmax()))
    return float(ratio.max())


def reference_loglike(res, var):
    """The reference's logL (rvmodel/__init__.py:78-80) of rows of residuals and variances; a NaN row of res is the invalid
    orbit's -1e30 (rvmodel:203)."""
    n = res.shape[1]
    cte = -0.5 * n * np.log(2 * np.pi)
    out = np.empty(res.shape[0])
    for b in range(res.shape[0]):
        out[b] = cte - np.sum(np.log(np.sqrt(var[b]))) - np.sum(res[b] ** 2 / (2 * var[b]))
    out[np.isnan(res).any(axis=1)] = -1e30
    return out


def prior_sets():
    z = np.load(GOLDEN / "priors.npz")
    meta = json.loads((GOLDEN / "priors.json").read_text())
    q = z["q"]
    return q, [(m["name"], m["args"], z[f"p{i}_ppf"], z[f"p{i}_raised"]) for i, m in enumerate(meta["sets"])]


# Kepler-solver cases: eccentricities, their mean anomalies and the itmax-abort case (gen_kepler_golden.py stores what the
# reference's own compiled trueanomaly() returns on exactly these inputs)
KEPLER_ECCS = (0.0, 0.05, 0.3, 0.6, 0.9, 0.95, 0.98, 0.99, 0.995, 1.3, -0.2)


def kepler_mean_anomalies(ecc):
    return np.random.default_rng(int(abs(ecc) * 1000)).uniform(-7.0e3, 7.0e3, 20000)


def kepler_itmax_mean_anomalies():
    return np.linspace(0.1, 3.0, 50)


def sha256(a):
    """Digest of an array's bytes: equal digests <=> bit-identical arrays (NaN payloads and signed zeros included)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def kepler_reference():
    """{ecc: dict(rc, m_sha256, nu_sha256, nu_sample)}, the sample index and the itmax case (nu, rc) of kepler_ref.npz."""
    z = np.load(GOLDEN / "kepler_ref.npz")
    cases = {float(e): dict(rc=int(z["rc"][i]), m_sha256=str(z["m_sha256"][i]), nu_sha256=str(z["nu_sha256"][i]),
                            nu_sample=z["nu_sample"][i]) for i, e in enumerate(z["ecc"])}
    return cases, z["sample_index"], (z["itmax_nu"], int(z["itmax_rc"]))


def rel_err(a, b):
    """|a-b| / max(|b|, 1e-300), elementwise; exact equality (incl. -1e30 sentinels, inf) counts as 0."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    err = np.where(a == b, 0.0, err)
    err = np.where(np.isnan(a) & np.isnan(b), 0.0, err)
    return err
