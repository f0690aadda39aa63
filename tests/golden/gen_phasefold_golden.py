#!/usr/bin/env python3
"""Golden-vector generator for the phase folds — runs ONLY in the build container, where the reference checkout is mounted at
/root/reference.  It imports the reference's own `evidence.rvmodel.RVModel` and walks the instruments as the phase-fold loop of
evidence/post_processing.py:396-444 does, calling the model's own kep_rv, modelk and drift, for the two shipped 51 Peg
configurations (the second with a linear drift) at one fixed parameter vector each, and writes

    phasefold_51peg.npz     per case: theta, and per epoch phase, rv (the corrected datum), rv_err, inst, model (the planet's
                            curve); t_ref and period

next to this file.  The reference never travels to the GPU box; the fixture does.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_phasefold_golden.py
"""
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True
np.int = int  # noqa: dev-only shim for the reference under numpy 2.x

from evidence.rvmodel import RVModel  # noqa: E402

import golden  # noqa: E402
from gen_golden import ref_datadict  # noqa: E402

warnings.filterwarnings("ignore")

THETA = {"hamilton_jitter": 3.0, "hamilton_offset": -2.0, "planet1_ecc": 0.05, "planet1_k1": 56.0, "planet1_ma0": 1.0,
         "planet1_omega": 0.7, "planet1_period": 4.2308, "drift_lin": 12.5}


def fold(model, pardict, n):
    period = pardict[f"planet{n}_period"]
    t_ref = 0
    ne = len(model.time)
    phase, rv, err, curve = np.zeros(ne), np.zeros(ne), np.zeros(ne), np.zeros(ne)
    for i, instrument in enumerate(model.insts):
        idx = np.where(model.data["inst_id"] == i)
        t, y = model.time[idx], model.vrad[idx]
        corrected = y - pardict[f"{instrument}_offset"]
        corrected -= model.kep_rv(pardict, t, exclude_planet=n)
        if model.drift_in_model:
            corrected -= model.drift(pardict, t)
        if model.linpar_in_model:
            for linpar in model.linpar_dict:
                corrected -= pardict[f"linpar_{linpar}"] * model.linpar_dict[linpar][idx]
        own = model.modelk(pardict, t, planet=n)
        yerr = model.svrad[idx]
        err[idx] = np.sqrt(yerr ** 2 + pardict[f"{instrument}_jitter"] ** 2) if model.jitter_in_model else yerr
        if t_ref == 0:
            t_ref = t[np.argmax(own)]
        phase[idx] = (((t - t_ref) / period) % 1. - 0.5) * period
        rv[idx], curve[idx] = corrected, own
    return dict(phase=phase, rv=rv, rv_err=err, inst=np.asarray(model.data["inst_id"], dtype=np.int32), model=curve,
                t_ref=float(t_ref), period=float(period))


if __name__ == "__main__":
    out = {}
    for case in golden.peg51_cases():
        model = RVModel(dict(case.fixed), ref_datadict(case.table), list(case.parnames))
        assert model.parnames == case.parnames
        theta = np.array([THETA[name] for name in model.parnames])
        pardict = {name: theta[i] for i, name in enumerate(model.parnames)}
        pardict.update(model.fixedpardict)
        got = fold(model, pardict, 1)
        out[f"{case.name}_theta"] = theta
        for key, val in got.items():
            out[f"{case.name}_{key}"] = np.asarray(val)
        print(case.name, "t_ref", got["t_ref"], "period", got["period"], "rv in", got["rv"].min(), got["rv"].max(),
              "drift" if model.drift_in_model else "no drift")
    np.savez_compressed(HERE / "phasefold_51peg.npz", **out)
    print("wrote", HERE / "phasefold_51peg.npz", (HERE / "phasefold_51peg.npz").stat().st_size, "bytes")
