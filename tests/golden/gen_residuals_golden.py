#!/usr/bin/env python3
"""Golden-vector generator for the residuals of the likelihood's model — runs ONLY in the build container, where the reference
checkout is mounted at /root/reference.  It imports the reference's own `evidence.rvmodel.RVModel` and repeats the lines of
RVModel.log_likelihood (evidence/rvmodel/__init__.py:180-215) up to `res` and `noise`, calling the model's own kep_rv and drift,
for the two shipped 51 Peg configurations (the second with a linear drift) at two parameter vectors each — the phase-fold
fixture's, and the same with the eccentricity at 0.6 — and writes

    residuals_51peg.npz     per case: theta [2, ndim], res [2, Ne], var [2, Ne], kep [2, Ne] (the Keplerian sum: the amplitude
                            the tests scale their bound with)

next to this file.  The reference never travels to the GPU box; the fixture does.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_residuals_golden.py
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
        assert kep is not None
        rvm += kep
    if model.drift_in_model:
        rvm += model.drift(pardict, model.time)
    if model.linpar_in_model:
        for linpar in model.linpar_dict:
            rvm += pardict[f"linpar_{linpar}"] * model.linpar_dict[linpar]
    return model.vrad - rvm, noise, kep


if __name__ == "__main__":
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
