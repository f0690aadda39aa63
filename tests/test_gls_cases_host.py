"""CPU: the yardstick of tests/test_gpu_gls_windows.py, checked without a device (tests/gls_cases.py).  gls_cases.window is
periodogram.gls_definition; the inputs meet their conditions from the long-double reference alone (no NaN at a compared frequency,
8 delta of every window within the project's parity bound where the geometry allows); a numpy emulation of the kernels'
arithmetic lies within 8 delta of every window of every case; each defect switched on in the emulation fails that bound, and
one of them would pass a single 8 delta taken over the whole long grid; rho = D / (CC SS) does not tell the cadence table's aliases
from sound frequencies, which is why nothing guards them."""
import numpy as np
import pytest

import gls_cases as gc
from evidence_amd import periodogram

_REF = {}


def _reference(case):
    if case.name not in _REF:
        time, res, var = case.host_rows()
        data = (time, res, var) + case.grid()
        _REF[case.name] = (data, gc.references(case, data))
    return _REF[case.name]


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["float64", "longdouble"])
def test_window_is_the_definition(dtype):
    case = gc.BY_NAME["gap65"]                                            # out of time order, ties
    time, res, var = case.host_rows()
    f0, df = case.grid()
    whole = periodogram.gls_definition(time, res, var, f0, df, 700, dtype=dtype)
    assert whole.dtype == dtype and np.all(np.isfinite(whole))
    assert np.array_equal(gc.window(time, res, var, f0, df, 0, 700, dtype=dtype), whole)
    assert np.array_equal(gc.window(time, res, var, f0, df, 512, 188, dtype=dtype), whole[:, 512:])
    for phase in gc.PHASES:
        assert np.array_equal(gc.window(time, res, var, f0, df, 0, 64, dtype=dtype, phase=phase),
                              periodogram.gls_definition(time, res, var, f0, df, 64, phase=phase, dtype=dtype))
    # the knobs move the result, and by rounding only
    base = gc.window(time, res, var, f0, df, 0, 64)
    for kw in (dict(order="sequential"), dict(order="reversed"), dict(nudge=1)):
        other = gc.window(time, res, var, f0, df, 0, 64, **kw)
        assert not np.array_equal(other, base) and np.max(np.abs(other - base)) <= 1e-12


def test_the_cases_are_the_ones_asked_for():
    names = [c.name for c in gc.CASES]
    assert len(set(names)) == len(names) == 2 + 2 * len(gc.NE_EDGES) + 2 + 3
    assert gc.NE_EDGES == (4, 5, 63, 64, 65, 255, 256, 257, 320, 513)
    for case in gc.CASES:
        time, res, var = case.host_rows()
        assert res.shape == (5, time.shape[0]) and np.all(var > 0) and all(k0 % 2 == 0 and k0 + nk <= case.F for k0, nk in case.windows)
        assert len(case.skip) * 100 <= case.F                             # at most 1 % left out
    assert gc.BY_NAME["51peg"].table.time.shape[0] == 256 and gc.BY_NAME["51peg"].F == (1 << 18) + 3
    assert np.all(np.diff(gc.BY_NAME["51peg"].table.time) >= 0)           # the 51 Peg table is in time order
    gap = gc.BY_NAME["gap65"].table.time
    assert np.all(np.diff(gc.BY_NAME["decreasing65"].table.time) < 0) and np.any(np.diff(gap) < 0) and np.unique(gap).shape[0] < 65
    assert np.any(np.diff(gc.BY_NAME["sinusoid"].table.time) < 0)
    two = gc.BY_NAME["two_svrad"].table
    assert sorted(set(np.asarray(two.svrad))) == [0.3, 30.0] and len(two.insts) == 2
    assert gc.BY_NAME["cadence65"].skip == (255, 511, 767, 1023, 1279, 1535, 1791, 2047, 2303)
    for case in gc.CASES:
        if case.name != "cadence65":
            assert case.skip == ()


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_the_emulation_lies_within_eight_delta_of_every_window(case):
    data, refs = _reference(case)
    time, res, var, f0, df = data
    span = float(time.max() - time.min())
    for win, d, wide in refs:
        keep = gc.kept(win, case.skip)
        # the conditions on the inputs, from the reference alone (gc.delta has asserted: finite at every kept frequency)
        assert d.shape == (5,) and np.all(d > 0.0)
        if not case.skip:
            assert np.all(np.isfinite(wide))
        if case.parity:
            assert gc.FACTOR * d.max() <= gc.PARITY, (case.name, win, d)
        got = gc.emulate(time, res, var, f0, df, win[0], win[1])
        r, whole = gc.ratio(got, wide, d, win, case.skip)
        print(f"{case.name} window {win[0]}+{win[1]} (f span up to {(f0 + df * (win[0] + win[1] - 1)) * span:.0f}): delta by row "
              f"{d.min():.1e} to {d.max():.1e}, emulation/delta of a row {r:.3f}, of the window {whole:.3f}, "
              f"peak {float(np.max(wide[:, keep])):.3f}")
        assert r <= gc.FACTOR, (case.name, win, r)
    if case.name == "sinusoid":
        assert all(float(np.max(wide[b])) > 0.9 for b in range(5) for win, d, wide in refs[:1])


DEFECT_CASES = ("51peg", "sorted5", "sorted65", "decreasing257", "gap65")


@pytest.mark.parametrize("name", DEFECT_CASES)
@pytest.mark.parametrize("defect", gc.DEFECTS)
def test_every_defect_fails_the_windowed_bound(defect, name):
    case = gc.BY_NAME[name]
    data, refs = _reference(case)
    time, res, var, f0, df = data
    worst, err, failed = 0.0, 0.0, []
    for win, d, wide in refs:
        got = gc.emulate(time, res, var, f0, df, win[0], win[1], defect=defect)
        r, _ = gc.ratio(got, wide, d, win, case.skip)
        worst, err = max(worst, r), max(err, float(np.max(gc.errors(got, wide, win, case.skip))))
        if r > gc.FACTOR:
            failed.append(win)
    one_delta = max(float(d.max()) for _, d, _ in refs)
    print(f"{defect} on {name}: largest ratio to a row's delta in a window {worst:.3g}, windows failed {failed}; largest error "
          f"{err:.3e} against one delta for the whole grid {one_delta:.3e} (ratio {err / one_delta:.3g})")
    assert worst > gc.FACTOR
    if defect == "short_polynomials" and name == "51peg":
        # up to 2e-13: inside 8 delta of the long grid as a whole, outside 8 delta of a row in the first window
        assert err <= gc.FACTOR * one_delta and (0, 512) in failed


def test_rho_does_not_separate_the_aliases_of_the_cadence_table():
    """rho = D / (CC SS) in long double at the cadence table's skipped entries against its smallest value over every compared
    entry of every case.  A guard on rho would need the two a factor of 100 apart; at an alias CC and SS are both rounding
    residue and rho is 1, -inf or NaN, so there is no such threshold and no code guards the aliases."""
    smallest, where = np.inf, None
    for case in gc.CASES:
        data, _ = _reference(case)
        for win in case.windows:
            rho = gc.rho_long_double(data, win)[:, gc.kept(win, case.skip)]
            assert np.all(np.isfinite(rho))
            if float(rho.min()) < smallest:
                smallest, where = float(rho.min()), (case.name, win)
    case = gc.BY_NAME["cadence65"]
    data, _ = _reference(case)
    at = gc.rho_long_double(data, (0, case.F))[:, list(case.skip)].astype(np.float64)
    print("smallest rho over every compared entry:", smallest, "at", where)
    print("rho at the skipped entries of the cadence table, by row:")
    for k, col in zip(case.skip, at.T):
        print("  k =", k, col)
    sound = np.isfinite(at) & (at > 0)
    assert smallest > 1e-5 and not np.all(sound & (at * 100.0 <= smallest))
    assert np.any(~sound) or float(np.max(at)) >= smallest               # some alias looks as sound as any frequency, or is NaN
