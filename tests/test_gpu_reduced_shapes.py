"""GPU: the reduced-precision modes (precision="mixed" / "fp32") at the small and odd shapes of tests/reduced_cases.py — one
item, ragged last rounds of a 256-thread tile (the pair is item i and item i + 256), LDS windows, the CU-wide form at one, two, an
odd and an even number of wave rounds, full and ragged (two tickets at once, the start round of tile_decode and its wrap), both
item paths (itmax 10000: pairs; itmax 16: single items), tol on both sides of the rotation and below what a float step can show
(every solve through the double solver), the itmax marks of the single-item path.

The reference is the fp64 oracle; the bound is four times the distance of a float32 restatement of the modes in numpy from
that oracle (reduced_cases.emulate, reduced_cases.bound: the margin is argued there), computed here on the host and never taken
from a device run; the geometry read back from the library tells the emulation which items share a wave and so stop together.  A lost, doubled or
mis-slotted item moves log-L by about 1 / (items of the row), >= 1e-4 at these shapes,
against bounds near 4e-7.  The median over the rows is held at the same margin: the emulation's medians are the device's
(0.93 .. 1.12 of them, profiles/reduced_shapes.txt; the fp32 medians recorded in tests/test_gpu_precision.py, a hundred times
larger, date from a float logarithm per item that the kernels no longer have)."""
import numpy as np
import pytest

import golden
import reduced_cases as rc
import solver_cases as sc
from evidence_amd import GpuRVModel, FLAG_INVALID_ORBIT, FLAG_NONCONVERGED
from evidence_amd import priors as P
from evidence_amd.synthetic import make_workload

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]
CU_THREADS = 1024


def _model(case, **kw):
    return GpuRVModel(case.fixed, case.table, case.parnames, linpar_dict=getattr(case, "linpar", None) or None, **kw)


def _set_form(m, form, pb):
    m.set_points_per_block(pb if form == "tile" else 0)
    m.set_kernel_form(form)


def _geometry(m, theta):
    """(threads, points per tile) of the launch the model's settings give this batch, read back from the library."""
    m.dev_reserve(theta.shape[0])
    m.dev_upload_theta(theta)
    t = m.dev_time_loglike(theta.shape[0], warmup=0, iters=1)
    return t["threads"], t["points_per_block"]


def _twice(m, theta):
    a = m.log_likelihood_batch(theta, return_flags=True)
    b = m.log_likelihood_batch(theta, return_flags=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the same launch twice: other bits"
    return a


def _check(label, case, y, got, flags, rflags, failures):
    err = golden.rel_err(got, y.ref)
    limit = rc.bound(case, y)
    print(f"RS| {label} | Y {y.max:.3e} median {y.median:.3e} | device max {err.max():.3e} median {np.median(err):.3e} "
          f"| device / bound {err.max() / limit:.3f} | device / Y {err.max() / max(y.max, rc.fp64_term(case)):.2f}")
    if not np.array_equal(flags, rflags):
        failures.append((label, "flags", np.flatnonzero(flags != rflags)[:8].tolist()))
    if not err.max() <= limit:
        failures.append((label, "max", float(err.max()), limit, int(err.argmax())))
    if not np.median(err) <= 4 * y.median + rc.fp64_term(case):
        failures.append((label, "median", float(np.median(err)), y.median))


RUNS = rc.runs()


@pytest.mark.parametrize("case, tol, itmax", RUNS, ids=[rc.run_id(*r) for r in RUNS])
def test_reduced_modes_at_edge_shapes(gpu_required, case, tol, itmax):
    """Both modes, at the case's own geometry and in the other kernel form: within reduced_cases.bound of the fp64 oracle, the
    oracle's flags (none), the same bits launch after launch; the tile the CU-wide form cuts is the one the case list counts on."""
    failures = []
    other = ("cu", 0) if case.form == "tile" else ("tile", 0)
    for precision in rc.PRECISIONS:
        with _model(case, precision=precision, tol=tol, itmax=itmax) as m:
            for form, pb in ((case.form, case.pb), other):
                _set_form(m, form, pb)
                threads, got_pb = _geometry(m, case.theta)
                # the yardstick of THIS launch: which items stop together is the geometry's (reduced_cases.pair_waves)
                y = rc.yardstick(case, precision, tol, itmax, ("cu" if threads == CU_THREADS else "tile", got_pb))
                assert not y.rflags.any()
                geo = f"{threads} threads x {got_pb} points"
                if form == "cu" and form == case.form:
                    want_pb, rounds, ragged = rc.cu_geometry(case.theta.shape[0], case.n_epochs)
                    assert (threads, got_pb) == (CU_THREADS, want_pb), (threads, got_pb, want_pb)
                    r0 = rc.wrap_start_rounds(case, got_pb)
                    geo += f", {rounds} rounds, {'ragged' if ragged else 'full'}, {int((r0 > 0).sum())} of {r0.size} tiles wrap"
                elif form == "tile" and form == case.form:
                    assert (threads, got_pb) == (256, case.pb)
                got, flags = _twice(m, case.theta)
                _check(f"{rc.run_id(case, tol, itmax)} {precision} {form} ({geo})", case, y, got, flags, y.rflags, failures)
    assert not failures, failures


@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_invalid_orbits_in_both_modes_and_forms(gpu_required, precision):
    """Every *_invalid case of the golden set: -1e30 and the fp64 path's flags, whatever the mode and the form."""
    cases = [c for c in golden.edge_cases() if c.name.endswith("_invalid")]
    assert cases
    for case in cases:
        with _model(case) as m:
            ref, rflags = m.log_likelihood_batch(case.theta, return_flags=True)
        assert np.all(ref == -1e30) and np.all(rflags & FLAG_INVALID_ORBIT)
        for itmax in (10000, 16):
            with _model(case, precision=precision, itmax=itmax) as m:
                for form in ("tile", "cu"):
                    _set_form(m, form, 0)
                    got, flags = _twice(m, case.theta)
                    assert np.all(got == -1e30) and np.array_equal(flags, rflags), (case.name, itmax, form)


def _one_launch_models():
    w = make_workload(3)
    cfg3 = dict(name="cfg3", table=w.table, parnames=list(w.parnames), fixed=dict(w.fixedpardict), priors=w.priordict(), nplanets=3)
    rng = np.random.default_rng(20)
    table, free, fixed, ranges, _ = rc._synthetic_case(rng, 150, 2, 2, False, 0, False)
    two = dict(name="two_planets", table=table, parnames=list(free), fixed=dict(fixed), nplanets=2,
               priors={nm: P.Uniform(*ranges[nm]) for nm in free})
    return [cfg3, two]


@pytest.mark.parametrize("which", [0, 1], ids=["cfg3", "two_planets"])
def test_one_launch_forms_in_both_modes(gpu_required, which):
    """cube -> theta -> log-L in one launch (cfg3: the three-planet fused-slim kernels; two planets: the generic loop) at 6, 40
    and 600 rows (zero-copy, pinned staging, plain), host buffers and device resident: theta is what prior_transform_batch
    returns, bit for bit, and log-L is within the bound of the oracle at that theta."""
    from types import SimpleNamespace
    spec = _one_launch_models()[which]
    cube = np.random.default_rng(31 + which).random((600, len(spec["parnames"])))
    failures = []
    for precision in rc.PRECISIONS:
        with GpuRVModel(spec["fixed"], spec["table"], spec["parnames"], priordict=spec["priors"], precision=precision) as m:
            theta2 = m.prior_transform_batch(cube)
            case = SimpleNamespace(name=f"one_launch_{spec['name']}", table=spec["table"], parnames=spec["parnames"], fixed=spec["fixed"],
                                   theta=np.ascontiguousarray(theta2), linpar={}, nplanets=spec["nplanets"])
            y = rc.yardstick(case, precision)                                   # at the device's own theta, all 600 rows
            for n in (6, 40, 600):
                theta, logl, flags = m.prior_loglike_batch(cube[:n], return_flags=True)
                m.dev_upload_cube(cube[:n])
                m.dev_prior_loglike(n)
                th3, ll3, fl3 = m.dev_download(n, theta=True, flags=True)
                assert np.array_equal(theta, theta2[:n]) and np.array_equal(th3, theta2[:n]), (precision, n)
                for label, got, fl in (("host", logl, flags), ("resident", ll3, fl3)):
                    err = golden.rel_err(got, y.ref[:n])
                    print(f"RS| one launch {spec['name']} {precision} {label} {n} rows | Y {y.max:.3e} | device max {err.max():.3e} "
                          f"median {np.median(err):.3e} | device / bound {err.max() / rc.bound(case, y):.3f}")
                    if not np.array_equal(fl, y.rflags[:n]):
                        failures.append((precision, label, n, "flags"))
                    if not err.max() <= rc.bound(case, y):
                        failures.append((precision, label, n, float(err.max()), rc.bound(case, y)))
    assert not failures, failures


@pytest.mark.parametrize("precision", rc.PRECISIONS)
def test_itmax_marks_of_the_single_item_path(gpu_required, precision):
    """itmax = 5 on the rows of solver_cases.placed(200, 256) where a float and a double solver abort each planet's array at the
    same epoch whatever the last bit of sin / cos (reduced_cases.placed_rows; the host file holds that they are most rows):
    the oracle's flags and log-L within the bound, in both forms and at several tilings — the mark sits anywhere in the array,
    the redo pass (3b) puts nu = 0 behind it."""
    case = rc.placed_kept_case()
    y = rc.yardstick(case, precision, 1e-4, sc.PLACED_ITMAX)
    assert (y.rflags & FLAG_NONCONVERGED).sum() >= 32
    failures = []
    with _model(case, precision=precision, itmax=sc.PLACED_ITMAX) as m:
        for form, pb in (("tile", 1), ("tile", 3), ("tile", 5), ("cu", 0)):
            _set_form(m, form, pb)
            got, flags = _twice(m, case.theta)
            _check(f"placed200_kept itmax 5 {precision} {form} pb {pb} ({case.theta.shape[0]} rows kept)", case, y, got, flags, y.rflags,
                   failures)
    assert not failures, failures
