#!/usr/bin/env python3
"""Golden-vector generator for the residuals of the likelihood's model — runs ONLY in the build container, where the reference
checkout is mounted at /root/reference.  It imports the reference's own `evidence.rvmodel.RVModel` and repeats the lines of
RVModel.log_likelihood (evidence/rvmodel/__init__.py:180-215) up to `res` and `noise`, calling the model's own kep_rv and drift,
for the two shipped 51 Peg configurations (the second with a linear drift) at two parameter vectors each — the phase-fold
fixture's, and the same with the eccentricity at 0.6 — and writes

    residuals_51peg.npz     per case: theta [2, ndim], res [2, Ne], var [2, Ne], kep [2, Ne] (the Keplerian sum: the amplitude
                            the tests scale their bound with)

    residuals_edges.npz     the same four arrays for the first 3 rows of every case of loglike_edges.npz, of the eccentricity sweep
                            and of the adversarial sweep (every parametrisation, drift order, tref rule, instrument count, linear
                            series and the no-jitter switch); an invalid orbit is a NaN row of res with its var

next to this file.  The reference never travels to the GPU box; the fixture does.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_residuals_golden.py [51peg] [edges]
"""
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(HERE))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
np.int = int  # noqa: dev-only shim for the reference under numpy 2.x

from evidence.rvmodel import RVModel  # noqa: E402

import golden  # noqa: E402
from gen_golden import ref_datadict  # noqa: E402
from gen_phasefold_golden import THETA  # noqa: E402

warnings.filterwarnings("ignore")

THETAS = (THETA, dict(THETA, planet1_ecc=0.6))


def residuals(model, pardict):
    """RVModel.log_likelihood up to `res` and `noise`, line by line."""
    noise = np.zeros_like(model.svrad)
    rvm = np.zeros_like(model.vrad)
    for i, instrument in enumerate(model.insts):
        inst_idxs = np.where(model.data["inst_id"] == i)
        rvm[inst_idxs] += pardict[f"{instrument}_offset"]
        if model.jitter_in_model:
            noise[inst_idxs] = model.svrad[inst_idxs] ** 2 + pardict[f"{instrument}_jitter"] ** 2
        else:
            noise[inst_idxs] = model.svrad[inst_idxs] ** 2
    kep = np.zeros_like(model.vrad)
    if model.nplanets > 0:
        kep = model.kep_rv(pardict, model.time)
        if kep is None:                      # an invalid orbit (log_likelihood returns -1e30 here): NaN res with its noise
            return np.full_like(model.vrad, np.nan), noise, np.full_like(model.vrad, np.nan)
        rvm += kep
    if model.drift_in_model:
        rvm += model.drift(pardict, model.time)
    if model.linpar_in_model:
        for linpar in model.linpar_dict:
            rvm += pardict[f"linpar_{linpar}"] * model.linpar_dict[linpar]
    return model.vrad - rvm, noise, kep


EDGE_ROWS = 3


def gen_edges():
    """residuals_edges.npz: for every case of loglike_edges.npz and for the eccentricity and the adversarial sweep, the first
    rows of theta: res, var, kep [3, Ne] and, where there is more than one planet, modelk of every planet at the epochs
    (pl1, pl2: what keep_planet leaves in; NaN where the reference returns None)."""
    from gen_golden import edge_models, ref_pardict
    models = list(edge_models())
    for case in (golden.high_ecc_case(), golden.wild_case()):
        models.append((case, RVModel(dict(case.fixed), ref_datadict(case.table), list(case.parnames))))
    out = {}
    for case, model in models:
        assert model.parnames == case.parnames and np.array_equal(model.time, case.table.time)
        theta = case.theta[:EDGE_ROWS]
        rows = [residuals(model, ref_pardict(model, x)) for x in theta]
        out[f"{case.name}_theta"] = theta
        for k, key in enumerate(("res", "var", "kep")):
            out[f"{case.name}_{key}"] = np.array([r[k] for r in rows])
        if model.nplanets > 1:
            for p in range(1, model.nplanets + 1):
                curves = [model.modelk(ref_pardict(model, x), model.time, planet=p) for x in theta]
                out[f"{case.name}_pl{p}"] = np.array([np.full_like(model.vrad, np.nan) if c is None else c for c in curves])
        print(f"{case.name:34s} {theta.shape[0]} rows, {int(np.isnan(out[case.name + '_res']).all(axis=1).sum())} NaN, planets",
              model.nplanets, "drift" if model.drift_in_model else "", "linpar" if model.linpar_in_model else "",
              "" if model.jitter_in_model else "no jitter")
    np.savez_compressed(HERE / "residuals_edges.npz", **out)
    print("wrote", HERE / "residuals_edges.npz", (HERE / "residuals_edges.npz").stat().st_size, "bytes")


def gen_51peg():
    out = {}
    for case in golden.peg51_cases():
        model = RVModel(dict(case.fixed), ref_datadict(case.table), list(case.parnames))
        assert model.parnames == case.parnames
        thetas, ress, noises, keps = [], [], [], []
        for values in THETAS:
            theta = np.array([values[name] for name in model.parnames])
            pardict = {name: theta[i] for i, name in enumerate(model.parnames)}
            pardict.update(model.fixedpardict)
            res, noise, kep = residuals(model, pardict)
            thetas.append(theta), ress.append(res), noises.append(noise), keps.append(kep)
            print(case.name, "ecc", values["planet1_ecc"], "res in", res.min(), res.max(), "var in", noise.min(), noise.max(),
                  "drift" if model.drift_in_model else "no drift")
        out[f"{case.name}_theta"] = np.array(thetas)
        out[f"{case.name}_res"] = np.array(ress)
        out[f"{case.name}_var"] = np.array(noises)
        out[f"{case.name}_kep"] = np.array(keps)
    np.savez_compressed(HERE / "residuals_51peg.npz", **out)
    print("wrote", HERE / "residuals_51peg.npz", (HERE / "residuals_51peg.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["51peg", "edges"]
    if "51peg" in which: gen_51peg()
    if "edges" in which: gen_edges()
