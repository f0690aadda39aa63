#!/usr/bin/env python3
"""Golden vectors of the reference's own Kepler solver: what its compiled trueanomaly() (oracle/_ref, built by
`make -C oracle ref` where the reference checkout is mounted) returns on the inputs of tests/golden.py's Kepler cases,
stored as tests/golden/kepler_ref.npz so that tests/test_oracle_golden.py pins the oracle's solver without the reference:

    ecc, rc, m_sha256, nu_sha256    per eccentricity: return code and the digests of the mean anomalies and of nu
    sample_index, nu_sample         64 fixed positions of every nu, for a readable failure
    itmax_nu, itmax_rc              the itmax-abort case in full (50 values)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_kepler_golden.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.dont_write_bytecode = True

import golden  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def main():
    if orc.load_ref() is None:
        sys.exit(f"{orc.REF_LIB} is missing: build it first (make -C oracle ref)")
    idx = np.random.default_rng(0).choice(20000, 64, replace=False)
    idx.sort()
    rc, m_sha, nu_sha, sample = [], [], [], []
    for ecc in golden.KEPLER_ECCS:
        M = golden.kepler_mean_anomalies(ecc)
        nu, r = orc.ref_trueanomaly(M, ecc)
        rc.append(r)
        m_sha.append(golden.sha256(M))
        nu_sha.append(golden.sha256(nu))
        sample.append(nu[idx])
    itmax_nu, itmax_rc = orc.ref_trueanomaly(golden.kepler_itmax_mean_anomalies(), 0.5, itmax=7, tol=0.0)
    np.savez_compressed(HERE / "kepler_ref.npz", ecc=np.array(golden.KEPLER_ECCS), rc=np.array(rc, dtype=np.int32),
                        m_sha256=np.array(m_sha), nu_sha256=np.array(nu_sha), sample_index=idx,
                        nu_sample=np.array(sample), itmax_nu=itmax_nu, itmax_rc=np.int32(itmax_rc))
    print(f"wrote {HERE / 'kepler_ref.npz'}: {len(rc)} eccentricities, return codes {rc}, itmax case rc {itmax_rc}")


if __name__ == "__main__":
    main()
