"""The GLS powers of the device (GpuRVModel.gls_bands / gls_batch; rvll_gls_bands, csrc/rvll_gls.hip) against the long-double
definition window by window (tests/gls_cases.py): on the grid the product uses — f0 = df = 1 / (8 span), 2^18 + 3
frequencies, so df * k0 at k0 = 262144, phases of 1e5 rad and 513 frequency tiles — on tables of 4 to 513 epochs in time order, in
decreasing time, in instrument order with ties and a 3000-day gap, with a sinusoid that brings the power to 1, with weights over
four decades, and at a 30-second cadence whose aliases of f = 0 lie on the grid.

Every case takes five rows (the 4-row tile has a tail), the device's own residuals_batch of them, and per window and row delta:
the largest distance from long double of twelve float64 evaluations of the definition (3 phase orders x 3 summation orders and
3 with every sin and cos nudged by an ulp).  The device must be finite where the reference is and within 8 delta of its row
and window; gls_bands and gls_batch must return the same bits.  delta comes from the definition alone.  On the cadence table
the nine frequencies at which every sine is 0 in exact arithmetic (gls_cases.CADENCE_SKIP, 0.39 % of its grid) are left out:
the definition is 0 / 0 there, in long double too, and neither it nor the device guards them.
Measured (profiles/gls_windows.txt): at most 1.02 delta of a row on the long grids, 1.53 elsewhere from 5 epochs up, 2.56 at 4
epochs, where the numpy emulation of the kernels gives 2.56 too."""
import numpy as np
import pytest

import gls_cases as gc
from evidence_amd import GpuRVModel
from test_gpu_merge import _51peg
from test_gpu_periodogram import _extras_model

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]

LEVELS = (0.15865, 0.5, 0.84135)


def _open(case):
    """(the case's model, theta [5, ndim])."""
    if case.model == "51peg":
        m = _51peg()
        return m, np.array(m.prior_transform_batch(np.random.default_rng(11).random((5, m.ndim))))
    if case.model == "extras":
        args, sample = _extras_model()
        return GpuRVModel(*args), sample(5, 11)
    m = GpuRVModel({}, case.table, gc.offsets_jitter_names(case.table))
    return m, gc.rows_theta(gc.offsets_jitter_rows(case.table), m.parnames)


def _check(case, power, data):
    """power [5, F] of the device against every window of the case; prints the largest ratio a window."""
    for win, d, wide in gc.references(case, data):
        k0, nk = win
        keep = gc.kept(win, case.skip)
        got = power[:, k0:k0 + nk]
        r, whole = gc.ratio(got, wide, d, win, case.skip)
        print(f"{case.name} window {k0}+{nk}: delta by row {d.min():.1e} to {d.max():.1e}, device/delta of a row {r:.3f}, "
              f"of the window {whole:.3f}")
        assert np.all(np.isfinite(got[:, keep])), (case.name, win)
        assert np.all(gc.errors(got, wide, win, case.skip) <= gc.FACTOR * d), (case.name, win, r)
    if case.skip:
        at = power[:, list(case.skip)]
        print(f"{case.name}: {int(np.isnan(at).sum())} of {at.size} powers at the skipped frequencies are NaN on the device; the "
              f"others lie in [{np.nanmin(at):.3g}, {np.nanmax(at):.3g}]")


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_powers_lie_within_eight_delta_of_every_window(gpu_required, case):
    f0, df = case.grid()
    m, theta = _open(case)
    with m:
        assert m.table.time.shape[0] == case.table.time.shape[0] and np.array_equal(m.table.time, case.table.time)
        res, var = m.residuals_batch(theta)
        got = m.gls_bands(theta[None], f0, df, case.F, LEVELS, return_power=True)
        batch = m.gls_batch(theta, f0, df, case.F)
    assert np.all(np.isfinite(res)) and np.all(var > 0)
    power = got["power"][0]
    assert power.shape == (5, case.F) and np.array_equal(batch, power, equal_nan=True)
    _check(case, power, (np.array(case.table.time, dtype=np.float64), res, var, f0, df))
    if case.name == "sinusoid":
        assert np.all(got["peak_power"][0] > 0.9) and np.all(power <= 1.0 + 1e-12)


def test_the_long_grid_in_two_chunks(gpu_required):
    """Two groups (the five rows, and the same rows in reverse) with chunk_bytes of one group: every group is a chunk of its own,
    and the powers are the bits of one call over both, held to the windows."""
    case = gc.BY_NAME["extras"]
    f0, df = case.grid()
    m, theta = _open(case)
    both = np.ascontiguousarray(np.stack([theta, theta[::-1]]))
    with m:
        ne = m.table.time.shape[0]
        res, var = m.residuals_batch(theta)
        whole = m.gls_bands(both, f0, df, case.F, LEVELS, return_power=True)
        split = m.gls_bands(both, f0, df, case.F, LEVELS, return_power=True, chunk_bytes=8 * 5 * (case.F + 2 * ne))
    for key in whole:
        assert np.array_equal(whole[key], split[key], equal_nan=True), key
    assert np.array_equal(split["power"][1], split["power"][0][::-1])
    _check(case, split["power"][1][::-1], (np.array(case.table.time, dtype=np.float64), res, var, f0, df))
