"""GPU: the device math the kernels are built from, checked in isolation through rvll_debug_eval."""
import numpy as np
import pytest

import math_cases as mc
from evidence_amd import GpuRVModel
from evidence_amd.synthetic import make_workload
from test_hostmath import hm  # noqa: F401  (the host build of the same headers, for the bit-for-bit test only)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]
ULP1 = 2.0 ** -53      # half-ulp of values in [1, 2) == one ulp of values in [0.5, 1)


@pytest.fixture(scope="module")
def dev(gpu_required):
    w = make_workload(1)
    m = GpuRVModel(w.fixedpardict, w.table, w.parnames)
    yield m
    m.close()


def test_div_exact_is_bit_identical_to_ieee_division(dev):
    """The Newton step E - f/f' must round exactly like the reference's division (trueanomaly.c:29)."""
    rng = np.random.default_rng(0)
    n = 4_000_000
    num = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 3, n)       # f = E - e sin E - M
    den = rng.uniform(0.01, 1.99, n)                                 # 1 - e cos E with e <= 0.99
    mine = dev.debug_eval(2, num, den)
    ieee = dev.debug_eval(3, num, den)
    assert np.array_equal(mine, ieee)
    assert np.array_equal(ieee, num / den)                           # and both equal the host's correctly rounded quotient


def test_div_fast_within_2ulp(dev):
    rng = np.random.default_rng(1)
    num = rng.normal(0, 50, 1_000_000)
    den = rng.uniform(0.01, 3000.0, 1_000_000)
    got = dev.debug_eval(4, num, den)
    ref = num / den
    assert np.max(np.abs(got - ref) / np.abs(ref)) <= 2.5 * 2.0 ** -52


def test_sincos_accuracy_over_the_unreduced_mean_anomaly_range(dev):
    """|M| reaches ~1e4 rad on this path (never range-reduced, rvmodel:459)."""
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(-2.0e4, 2.0e4, 2_000_000), rng.uniform(-7, 7, 500_000),
                        np.round(rng.uniform(-2.0e4, 2.0e4, 200_000) / (np.pi / 2)) * (np.pi / 2)])
    xl = x.astype(np.longdouble)
    s, c = dev.debug_eval(0, x), dev.debug_eval(1, x)
    es = np.max(np.abs(s.astype(np.longdouble) - np.sin(xl)))
    ec = np.max(np.abs(c.astype(np.longdouble) - np.cos(xl)))
    assert es <= 1.5 * ULP1 and ec <= 1.5 * ULP1, (float(es / ULP1), float(ec / ULP1))


def test_rotate_small_matches_direct(dev):
    rng = np.random.default_rng(3)
    x = rng.uniform(-10, 10, 500_000)
    h = rng.uniform(-1e-3, 1e-3, 500_000)
    xl, hl = x.astype(np.longdouble), h.astype(np.longdouble)
    s, c = dev.debug_eval(8, x, h), dev.debug_eval(9, x, h)
    ref_s = np.sin(xl) * np.cos(hl) + np.cos(xl) * np.sin(hl)
    ref_c = np.cos(xl) * np.cos(hl) - np.sin(xl) * np.sin(hl)
    assert np.max(np.abs(s.astype(np.longdouble) - ref_s)) <= 2.5 * ULP1
    assert np.max(np.abs(c.astype(np.longdouble) - ref_c)) <= 2.5 * ULP1


def test_log_pos_accuracy(dev):
    rng = np.random.default_rng(4)
    v = np.concatenate([10.0 ** rng.uniform(-6, 8, 1_000_000), rng.uniform(0.25, 2500.0, 1_000_000),
                        [1.0, 0.5, 2.0, 0.7071067811865476, 1.4142135623730951, 5e-324, 1e-310, 1e308]])
    got = dev.debug_eval(5, v)
    ref = np.log(v.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - ref) / np.maximum(np.abs(ref), np.longdouble(1e-300))
    absr = np.abs(got.astype(np.longdouble) - ref)
    assert np.max(np.minimum(err, absr)) <= 2.5 * 2.0 ** -52
    special = dev.debug_eval(5, np.array([0.0, -1.0, np.inf, np.nan]))
    assert special[0] == -np.inf and np.isnan(special[1]) and special[2] == np.inf and np.isnan(special[3])


def test_ndtri_against_scipy(dev):
    from scipy.special import ndtri
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(500_000), 10.0 ** rng.uniform(-300, -1, 100_000), 1 - 10.0 ** rng.uniform(-15, -1, 100_000),
                        [0.0, 1.0, 0.5, 0.075, 0.925]])
    got = dev.debug_eval(7, p)
    ref = ndtri(p)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin])
    err = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
    err = np.where(ref[fin] == 0, np.abs(got[fin]), err)
    assert err.max() <= 1e-13, float(err.max())


def test_lane0_tree_without_lds_crossbar_is_the_shuffle_tree(dev):
    """The per-point reduction ends in a 6-step tree over the wave.  The kernels take lane 0's value from a
    v_permlane32_swap / v_permlane16_swap / row_shl-DPP form of it; it must be the shuffle tree bit for bit, and
    both must be the tree as written: v[i] += v[i + off] for off = 32, 16, 8, 4, 2, 1."""
    rng = np.random.default_rng(12)
    n = 256 * 512
    x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-12, 12, n)
    shfl = dev.debug_eval(12, x)[::64]
    fast = dev.debug_eval(13, x)[::64]
    v = x.reshape(-1, 64).copy()
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
    assert np.array_equal(shfl, v[:, 0])
    assert np.array_equal(fast, v[:, 0])


def test_device_sincos_cr_is_correctly_rounded(dev):
    """The redo pass's sin / cos pair ON THE DEVICE (debug_eval 20 / 21: rvll_math.h sincos_cr — double-double reduction, table
    route with Ziv's test, full series where it declines) against mpmath at 200 bits: every value THE nearest double, from
    1e-300 to 1e300, next to multiples of pi/2 included (the host compilation of the same header: tests/test_hostmath.py)."""
    import math
    import mpmath
    mpmath.mp.prec = 200
    rng = np.random.default_rng(21)
    x = np.concatenate([rng.uniform(-20, 20, 4000), 10.0 ** rng.uniform(-300, 300, 1000) * rng.choice([-1, 1], 1000),
                        rng.uniform(1e9, 2e22, 3000), np.arange(1, 300) * (math.pi / 2), np.arange(0, 52) / 64.0,
                        np.array([0.0, 0.7853981633974483, -0.7853981633974483, 1e22, 2.0 ** 50, 2.0 ** 1023])])
    s, c = dev.debug_eval(20, x), dev.debug_eval(21, x)
    want_s = np.array([float(mpmath.sin(mpmath.mpf(float(v)))) for v in x])
    want_c = np.array([float(mpmath.cos(mpmath.mpf(float(v)))) for v in x])
    assert np.array_equal(s, want_s) and np.array_equal(c, want_c)


# ---- the rest of rvll_math.h on the device: debug_eval 22 - 35 (vectors, references and bounds: tests/math_cases.py) -----------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _device_long_route(dev, x):
    """sincos_any's long route wherever reduce_huge is valid (|x| >= 2^-10), not only beyond the switch: reduce_huge on the
    device (24 / 25), the kernels on its r (op 0 / 1: for |r| <= pi/4 sincos_f64 is its kernels), the quadrant put on here."""
    r, q = dev.debug_eval(24, x), dev.debug_eval(25, x)
    assert np.all(np.abs(r) <= 0.7853981633974484) and np.all((q >= 0) & (q <= 3) & (q == np.floor(q)))
    return mc.quadrant(x, r, q, dev.debug_eval(0, r), dev.debug_eval(1, r))


@pytest.mark.parametrize("band", mc.BANDS, ids=lambda b: f"2^{b[0]}-2^{b[1]}")
def test_sincos_f64_by_band_up_to_its_switch(dev, band):
    """sincos_f64 from 2^14 to its switch at 2^50 (the inline-asm Horner chains, v_bfi, bitop3): log-uniform arguments of both
    signs and the doubles next to multiples of pi/2, against long-double libm.  1.5 * 2^-53 below 2^48; in the two bands above,
    what the host build measures against mpmath on the same vector (1.12 and 4.23: math_cases.HOST_TOP_BAND, held by
    test_hostmath.py) plus 0.5 for the reference's rounding.  Measured on the MI355X: see profiles/math_primitives.txt."""
    x = mc.band_vector(*band)
    s, c = dev.debug_eval(0, x), dev.debug_eval(1, x)
    rs, rc = mc.band_reference(*band)
    es = float(np.max(np.abs(s.astype(np.longdouble) - rs))) / mc.ULP53
    ec = float(np.max(np.abs(c.astype(np.longdouble) - rc))) / mc.ULP53
    print(f"device sincos_f64 2^{band[0]}..2^{band[1]}: sin {es:.3f} cos {ec:.3f} (2^-53), n = {x.size}")
    assert es <= mc.band_bound(band) and ec <= mc.band_bound(band), (band, es, ec)


def test_sincos_any_on_the_device(dev):
    """sincos_any as the device compiles it (__umul64hi, the constant-memory 2/pi table, the device's ldexp and clz) on the vector
    of test_hostmath.py::test_sincos_of_any_finite_double, [2^49, 2^50) weighed with 2e4 arguments: that test's bounds against
    glibc; the long route relatively accurate where sin is tiny; inf / nan give nan; below 2^50 the very bits of sincos_f64 (what
    lets the shortcut loop and sincos_any share a tile); and across the switch the long route against mpmath."""
    import mpmath
    x, _ = mc.any_vector()
    rs, rc = mc.any_reference()
    ulp = 2.0 ** -52
    s, c = dev.debug_eval(22, x), dev.debug_eval(23, x)
    bound = mc.any_bound()
    es, ec = np.abs(s - rs), np.abs(c - rc)
    assert np.all(es <= bound), (float(np.max(es / bound)), float(x[np.argmax(es / bound)]))
    assert np.all(ec <= bound), (float(np.max(ec / bound)), float(x[np.argmax(ec / bound)]))
    short = np.abs(x) < 2.0 ** 50
    assert short.sum() > 20000 and (~short).sum() > 20000
    assert np.array_equal(_bits(s[short]), _bits(dev.debug_eval(0, x)[short]))
    assert np.array_equal(_bits(c[short]), _bits(dev.debug_eval(1, x)[short]))
    # the long route by itself from 1 upwards, where the short one is valid too
    sel = np.abs(x) >= 1.0
    xs = np.ascontiguousarray(x[sel])
    sl, cl = _device_long_route(dev, xs)
    el, ecl = np.abs(sl - rs[sel]), np.abs(cl - rc[sel])
    assert el.max() <= 1.5 * ulp and ecl.max() <= 1.5 * ulp, (float(el.max() / ulp), float(ecl.max() / ulp))
    tiny = np.abs(rs[sel]) < 1e-6
    assert tiny.sum() > 100
    assert np.max(el[tiny] / np.abs(rs[sel][tiny])) <= 4 * ulp
    big = np.abs(xs) >= 2.0 ** 50                            # ... and there it IS what sincos_any returns
    assert np.array_equal(_bits(sl[big]), _bits(s[sel][big])) and np.array_equal(_bits(cl[big]), _bits(c[sel][big]))
    bad = np.array([np.inf, -np.inf, np.nan])
    assert np.isnan(dev.debug_eval(22, bad)).all() and np.isnan(dev.debug_eval(23, bad)).all()
    # across the switch
    xw = mc.switch_vector()
    sw, cw = _device_long_route(dev, xw)
    with mpmath.workprec(160):
        ws = max(abs(mpmath.sin(mpmath.mpf(v)) - g) for v, g in zip(xw.tolist(), sw.tolist()))
        wc = max(abs(mpmath.cos(mpmath.mpf(v)) - g) for v, g in zip(xw.tolist(), cw.tolist()))
    assert float(ws) <= 1.5 * mc.ULP53 and float(wc) <= 1.5 * mc.ULP53, (float(ws) / mc.ULP53, float(wc) / mc.ULP53)


def test_device_is_the_host_build_bit_for_bit(dev, hm):  # noqa: F811
    """sincos_any, reduce_huge, sincos_f32, sincos_f32x2 and reduce_2pi_to_f32 hold no device-only arithmetic beyond bit selects:
    the device returns the bits of the host compilation of the same header, and each component of the packed pair the bits of
    the scalar routine."""
    x, _ = mc.any_vector()
    x = np.concatenate([x, mc.switch_vector(), [np.inf, -np.inf, np.nan, 0.0, -0.0, 1e-300]])
    hs, hc = mc.host_call(hm, "hm_sincos_any", [x], 2)
    assert _same_bits(dev.debug_eval(22, x), hs) and _same_bits(dev.debug_eval(23, x), hc)
    hr, hq = mc.host_call(hm, "hm_reduce_huge", [x], 2)
    assert np.isfinite(hr).sum() > 60000
    assert _same_bits(dev.debug_eval(24, x), hr) and _same_bits(dev.debug_eval(25, x), hq)
    for b in mc.BANDS:
        xb = mc.band_vector(*b)
        hs, hc = mc.host_call(hm, "hm_sincos_any", [xb], 2)
        assert _same_bits(dev.debug_eval(22, xb), hs) and _same_bits(dev.debug_eval(23, xb), hc), b
    f = mc.f32_vector()
    g = np.ascontiguousarray(f[::-1])
    hs, hc = mc.host_call(hm, "hm_sincos_f32", [f], 2)
    ds, dc = dev.debug_eval(26, f), dev.debug_eval(27, f)
    assert _same_bits(ds, hs) and _same_bits(dc, hc)
    pair = [dev.debug_eval(op, f, g) for op in (28, 29, 30, 31)]
    assert _same_bits(pair[0], ds) and _same_bits(pair[1], ds[::-1]) and _same_bits(pair[2], dc) and _same_bits(pair[3], dc[::-1])
    for got, want in zip(pair, mc.host_call(hm, "hm_sincos_f32x2", [f, g], 4)):
        assert _same_bits(got, want)
    for xr in (mc.reduce_vector(), mc.reduce_edge_vector(), mc.band_vector(14, 30)):
        assert _same_bits(dev.debug_eval(32, xr), mc.host_call(hm, "hm_reduce_2pi_to_f32", [xr], 1)[0])


def test_sincos_f32_accuracy_on_the_device(dev):
    """sincos_f32 and both components of sincos_f32x2 on 2e6 floats in [-8, 8] and every float within 4 ulps of k pi/2,
    |k| <= 5, against float64 libm: 1.5 * 2^-24 absolute.  (With the pi/2 split these routines had before — FreeBSD's 25-bit
    pio2_1, a tie as a float, one ulp lost per quadrant passed — this fails: sin 4.56, cos 5.17 on this vector.)"""
    x = mc.f32_vector()
    y = np.ascontiguousarray(x[::-1])
    rs, rc = mc.f32_reference()
    for name, s, c in (("sincos_f32", dev.debug_eval(26, x), dev.debug_eval(27, x)),
                       ("sincos_f32x2.x", dev.debug_eval(28, x, y), dev.debug_eval(30, x, y)),
                       ("sincos_f32x2.y", dev.debug_eval(29, y, x), dev.debug_eval(31, y, x))):
        assert np.array_equal(s, s.astype(np.float32)) and np.array_equal(c, c.astype(np.float32))      # floats, widened
        es, ec = np.max(np.abs(s - rs)) / mc.ULP24, np.max(np.abs(c - rc)) / mc.ULP24
        print(f"device {name}: sin {es:.3f} cos {ec:.3f} (2^-24)")
        assert es <= mc.SINCOS_F32_BOUND and ec <= mc.SINCOS_F32_BOUND, (name, float(es), float(ec))


def test_reduce_2pi_to_f32_on_the_device(dev):
    """reduce_2pi_to_f32 against the reduction in mpmath rounded to float, |x| <= 2e4 dense and log-uniform to 2^48:
    |r| <= float(pi) (1 + 2^-23), |r - true| <= ulp_f32(true) / 2 + |x| 2^-100 + 2^-53; and next to half-integers of x / (2 pi) at
    large |x|, where the routine's 1 / (2 pi) picks the wrong neighbour, r still x modulo 2 pi and beyond pi by no more than that
    constant's error allows."""
    x = mc.reduce_vector()
    r = dev.debug_eval(32, x)
    assert np.array_equal(r, r.astype(np.float32))
    over, at, rmax = mc.check_reduce_2pi(x, r)
    assert rmax <= mc.R2PI_MAX, rmax
    assert over <= 0, (over, at)
    x = mc.reduce_edge_vector()
    r = dev.debug_eval(32, x)
    over, at, _ = mc.check_reduce_2pi(x, r)
    assert over <= 0, (over, at)
    assert np.all(np.abs(r) <= mc.reduce_edge_range(x)), float(np.max(np.abs(r)))


def test_div_f32_within_one_ulp_of_ieee_division(dev):
    """div_f32 and both components of div_f32x2 (v_rcp_f32, good to 1 ulp, and one residual step) within one float ulp of the
    IEEE float quotient, for n ~ N(0, 1) 10^[-6, 3] over d in [0.01, 1.99]; the share that is not bit-equal is printed
    (profiles/math_primitives.txt)."""
    n, d = mc.div_vector()
    n0, n1, d0, d1 = mc.div_pair_operands()
    for name, got, nn, dd in (("div_f32", dev.debug_eval(33, n, d), n0, d0), ("div_f32x2.x", dev.debug_eval(34, n, d), n0, d0),
                              ("div_f32x2.y", dev.debug_eval(35, n, d), n1, d1)):
        assert np.array_equal(got, got.astype(np.float32))
        off, share = mc.div_ulps_off(got, nn, dd)
        print(f"device {name}: at most {off:.2f} ulp from IEEE, {100 * share:.4f} % not bit-equal")
        assert off <= 1.0, (name, off)


@pytest.fixture(scope="module")
def clamp_fp64(gpu_required):
    """The fp64 path on every 64th point of the clamp sweep, for both item paths' itmax."""
    fixed, table, parnames, theta = mc.clamp_sweep()
    out = {}
    for itmax in (10000, 16):
        with GpuRVModel(fixed, table, parnames, itmax=itmax) as m:
            out[itmax] = m.log_likelihood_batch(np.ascontiguousarray(theta[::64]))
    return out


@pytest.mark.parametrize("itmax", [10000, 16], ids=["pairs", "single"])
@pytest.mark.parametrize("precision", ["mixed", "fp32"])
def test_fp32_newton_loops_hand_every_unsettled_solve_to_double(clamp_fp64, precision, itmax):
    """2^27 solves at the eccentricity clamp with M modulo 2 pi dense in [-pi, pi], through the packed pair loop (the reference's
    itmax) and the single-item loop (itmax = 16): every log-L finite, and every 64th point within the modes' class (0.1, as
    test_reduced_precision_does_not_fall_apart_at_the_eccentricity_clamp has it) of the fp64 path.  At the clamp a float iterate
    is thrown out to 1e5 .. 1e12, beyond sincos_f32's reduction: the polynomials return 1e20 and more, and either the step
    f / f' vanishes and the iterate "settles" at a nonsense E, or it overflows and the next step is NaN, which fails every
    |dE| > tol.  The loops take a solve for settled only with |dE| <= tol and |E - M| <= 1 + tol, every test NaN-safe, and hand
    the others to the double solve.  Before that this sweep returned 21 NaN points of 65536 through the pair loop (none through
    the single-item loop) and its finite ones were up to 2.3e-2 from fp64; now 3.5e-8 (pairs) and 1.0e-2 (single: itmax = 16
    cuts wandering solves short in both precisions, at different epochs).  profiles/math_primitives.txt."""
    import golden
    fixed, table, parnames, theta = mc.clamp_sweep()
    with GpuRVModel(fixed, table, parnames, precision=precision, itmax=itmax) as m:
        got = m.log_likelihood_batch(theta)
    bad = int(np.count_nonzero(~np.isfinite(got)))
    err = golden.rel_err(got[::64], clamp_fp64[itmax])
    print(f"clamp sweep {precision} itmax={itmax}: {bad} of {got.size} log-L not finite; against fp64 max {np.nanmax(err):.3e}")
    assert bad == 0, bad
    assert err.max() <= 0.1, float(err.max())
