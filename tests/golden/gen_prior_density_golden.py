#!/usr/bin/env python
"""Golden log densities of the reference's priors — runs ONLY where the reference checkout is mounted at /root/reference.

For every family of the reference's `distdict` except UniformFrequency, Log10Normal (their `.pdf` are not the density of the
transform: tests/test_prior_density_host.py pins them by their own statements) and the two sorted kinds (pypolychord), and at
least two argument sets a family, the reference's `.logpdf` at about 200 points inside the support, at both ends of a finite
support and at points outside on both sides.  Written to tests/golden/prior_density.npz (x<i>, v<i> per case) and
prior_density.json (the cases' names and arguments, in order).

The JSON also records, per case, how well the reference's own `.ppf` and `.pdf` agree ("consistency"): q = linspace(0.001,
0.999, 65) goes through `.ppf` (one scalar at a time: the table kinds take no arrays), exp(logpdf) is integrated between
consecutive values with Simpson's rule on 65 points, and the largest |integral - (q[i + 1] - q[i])| is kept.  The device test
of the transform against the density (tests/test_gpu_prior_density.py) takes its bounds from these.

Left out are the points where the reference's own value is an artefact: Sine at exactly 0 or 180 (ln sin pi is -41 by
rounding), an open end where the reference gives +inf or NaN instead of -inf (Beta at 0 with a < 1; Alpha at 0), and anything
within 1e-6 of a support end other than the end itself.  Alpha's points start at 0.05: below about 0.03 the reference's pdf
underflows and its logpdf, the log of that, is -inf where the density is not zero.
"""
import json
import sys
import warnings
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, "/root/reference")
np.int = int  # noqa: dev-only shim for the reference under numpy 2.x

from evidence import priors as ref  # noqa: E402

INF = float("inf")
# (name, args, support lo, support hi, the range the interior points span)
CASES = [
    ("Uniform", (0.0, 20.0), 0.0, 20.0, None),
    ("Uniform", (-3.5, 1.25), -3.5, 1.25, None),
    ("Jeffreys", (10.0, 100.0), 10.0, 100.0, None),
    ("Jeffreys", (0.01, 2000.0), 0.01, 2000.0, None),
    ("ModJeffreys", (1.0, 999.0), 0.0, 999.0, None),
    ("ModJeffreys", (0.5, 30.0), 0.0, 30.0, None),
    ("Normal", (0.0, 1.0), -INF, INF, (-8.0, 8.0)),
    ("Normal", (51050.0, 12.5), -INF, INF, (50950.0, 51150.0)),
    ("LogNormal", (0.5, 0.0, 2.0), 0.0, INF, (0.0, 30.0)),
    ("LogNormal", (1.5, -1.0, 0.3), -1.0, INF, (-1.0, 40.0)),
    ("Binormal", (0.0, 1.0, 5.0, 2.0, 0.3), -INF, INF, (-8.0, 20.0)),
    ("Binormal", (-2.0, 0.5, -1.0, 0.25, -0.6), -INF, INF, (-6.0, 1.0)),
    ("Binormal", (0.0, 1.0, 3.0, 1.0, 1.0), -INF, INF, (-6.0, 9.0)),
    ("AsymmetricNormal", (0.0, 1.0, 3.0), -INF, INF, (-8.0, 24.0)),
    ("AsymmetricNormal", (10.0, 2.5, 0.5), -INF, INF, (-10.0, 14.0)),
    ("TruncatedUNormal", (0.0, 1.0, -1.0, 2.0), -1.0, 2.0, None),
    ("TruncatedUNormal", (5.0, 0.5, 4.5, 9.0), 4.5, 9.0, None),
    ("TruncatedRayleigh", (0.2, 1.0), 0.0, 1.0, None),
    ("TruncatedRayleigh", (3.0, 4.0), 0.0, 4.0, None),
    ("PowerLaw", (-2.0, 1.0, 10.0), 1.0, 10.0, None),
    ("PowerLaw", (0.5, 0.0, 3.0), 0.0, 3.0, None),
    ("DoublePowerLaw", (-1.5, -3.0, 5.0, 1.0, 100.0), 1.0, 100.0, None),
    ("DoublePowerLaw", (0.5, -2.0, 2.0, 0.5, 20.0), 0.5, 20.0, None),
    ("Sine", (0.0, 180.0), 0.0, 180.0, None),
    ("Sine", (10.0, 90.0), 10.0, 90.0, None),
    ("Sine", (-20.0, 120.0), 0.0, 120.0, None),
    ("Alpha", (2.0,), 0.0, INF, (0.05, 5.0)),
    ("Alpha", (0.7,), 0.0, INF, (0.05, 40.0)),
    ("Beta", (0.867, 3.03), 0.0, 1.0, None),
    ("Beta", (2.0, 5.0), 0.0, 1.0, None),
    ("Beta", (3.5, 0.9), 0.0, 1.0, None),
    ("Gamma", (2.0, 3.0), 0.0, INF, (0.0, 8.0)),
    ("Gamma", (5.5, 0.5), 0.0, INF, (0.0, 60.0)),
]
MARGIN = 1e-6


def points(lo, hi, span, rng):
    a, b = (lo, hi) if span is None else span
    width = b - a
    inner = np.concatenate([np.linspace(a + 1e-3 * width, b - 1e-3 * width, 150), rng.uniform(a + 1e-3 * width, b - 1e-3 * width, 50)])
    extra = []
    if np.isfinite(lo):
        extra += [lo, lo - 1e-3 * width, lo - 0.5 * width, lo - 10.0 * width]
    if np.isfinite(hi):
        extra += [hi, hi + 1e-3 * width, hi + 0.5 * width, hi + 10.0 * width]
    return np.concatenate([inner, extra])


def simpson_steps(theta, logpdf):
    """The integral of exp(logpdf) between consecutive theta, Simpson's rule on 65 points each."""
    x = np.linspace(theta[:-1], theta[1:], 65, axis=1)                       # [64, 65]
    with np.errstate(all="ignore"):
        f = np.exp(logpdf(x.reshape(-1))).reshape(x.shape)
    h = (theta[1:] - theta[:-1]) / 64.0
    return h / 3.0 * (f[:, 0] + 4.0 * f[:, 1:-1:2].sum(axis=1) + 2.0 * f[:, 2:-1:2].sum(axis=1) + f[:, -1])


def consistency(name, args):
    q = np.linspace(0.001, 0.999, 65)
    dist = getattr(ref, name)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        theta = np.array([float(dist.ppf(float(qi), *args)) for qi in q])
        steps = simpson_steps(theta, lambda x: dist.logpdf(x, *args))
    return float(np.max(np.abs(steps - np.diff(q))))


def main():
    rng = np.random.default_rng(20261020)
    arrays, cases = {}, []
    for i, (name, args, lo, hi, span) in enumerate(CASES):
        x = points(lo, hi, span, rng)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            v = np.asarray(getattr(ref, name).logpdf(x, *args), dtype=np.float64)
        end = (x == lo) | (x == hi)
        near = ((np.abs(x - lo) <= MARGIN) | (np.abs(x - hi) <= MARGIN)) & ~end
        keep = ~near
        if name == "Sine":
            keep &= ~((x == 0.0) | (x == 180.0))
        keep &= ~(end & (np.isnan(v) | (v == INF)))                # an open end the reference does not give -inf at
        assert not np.isnan(v[keep]).any() and not (v[keep] == INF).any(), name
        arrays[f"x{i}"], arrays[f"v{i}"] = x[keep], v[keep]
        cases.append({"name": name, "args": list(args), "lo": lo if np.isfinite(lo) else None, "hi": hi if np.isfinite(hi) else None,
                      "consistency": consistency(name, args)})
        print(f"{name}{args}: {int(keep.sum())} points, {int(np.isfinite(v[keep]).sum())} inside; ppf against pdf "
              f"{cases[-1]['consistency']:.2e}")
    np.savez_compressed(HERE / "prior_density.npz", **arrays)
    (HERE / "prior_density.json").write_text(json.dumps({"cases": cases}, indent=1) + "\n")


if __name__ == "__main__":
    main()
