"""Argument vectors, references and recorded figures shared by the math tests of the host build (tests/test_hostmath.py)
and of the device (tests/test_gpu_math.py).  Every vector is seeded and cached: both sides see the very same arguments,
and a reference is computed once per session."""
import ctypes as C
import functools
import math

import numpy as np

ULP53 = 2.0 ** -53                   # half an ulp of doubles in [1, 2) == one ulp of doubles in [0.5, 1)
ULP24 = 2.0 ** -24                   # the same for floats
PIO2_L = np.longdouble(1.5707963267948966) + np.longdouble(6.123233995736766e-17)      # pi/2 to the long double's 64 bits
dp = C.POINTER(C.c_double)

# ---- sincos_f64 by band ---------------------------------------------------------------------------------------------------
BANDS = [(14, 30), (30, 40), (40, 46), (46, 48), (48, 49), (49, 50)]
SINCOS_F64_BOUND = 1.5               # units of 2^-53, below 2^48
# Above 2^48 the rounding of the 2/pi constant itself moves x * 2/pi (by up to ~0.04 at 2^50): k can be the wrong neighbour,
# |r| reaches 0.85 and the minimax kernels degrade outside [-pi/4, pi/4].  The bound there is what the HOST build of the same
# operations in the same order measures against mpmath on the band's vector (max of sin and cos, units of 2^-53, rounded up;
# test_hostmath.py::test_sincos_f64_top_bands_against_mpmath holds the figures), plus 0.5 for the reference's own rounding.
HOST_TOP_BAND = {(48, 49): 1.12, (49, 50): 4.23}
REFERENCE_ROUNDING = 0.5


def band_bound(band):
    return HOST_TOP_BAND[band] + REFERENCE_ROUNDING if band in HOST_TOP_BAND else SINCOS_F64_BOUND


@functools.lru_cache(maxsize=None)
def band_vector(lo, hi):
    """Log-uniform arguments of both signs in [2^lo, 2^hi) and the doubles nearest to multiples of pi/2 there.  The top two
    bands hold 2e4 values in all (their host figure is measured with mpmath), the others 5e5."""
    n_rand, n_near = (16000, 4000) if (lo, hi) in HOST_TOP_BAND else (400000, 100000)
    rng = np.random.default_rng(1000 + lo)
    x = 2.0 ** rng.uniform(lo, hi, n_rand)
    k = rng.integers(math.ceil(2.0 ** lo / (math.pi / 2)) + 1, math.floor(2.0 ** hi / (math.pi / 2)), n_near)
    near = (k.astype(np.longdouble) * PIO2_L).astype(np.float64)
    x = np.concatenate([x, near])
    x = x * rng.choice([-1.0, 1.0], x.size)
    assert np.all((np.abs(x) >= 2.0 ** lo) & (np.abs(x) < 2.0 ** hi))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def band_reference(lo, hi):
    xl = band_vector(lo, hi).astype(np.longdouble)
    return np.sin(xl), np.cos(xl)


def err_vs_mpmath(x, s, c):
    """max |s - sin x|, max |c - cos x| with the true values from mpmath (no rounding of the reference), as floats."""
    import mpmath
    with mpmath.workprec(160):
        es = ec = mpmath.mpf(0)
        for xv, sv, cv in zip(x.tolist(), s.tolist(), c.tolist()):
            t = mpmath.mpf(xv)
            es = max(es, abs(mpmath.sin(t) - sv))
            ec = max(ec, abs(mpmath.cos(t) - cv))
        return float(es), float(ec)


# ---- sincos_any -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def any_vector():
    """(x, band): random arguments up to 1e300, exact powers of two, around the switch at 2^50, known hard cases, the doubles
    next to multiples of pi and pi/2 — and, as band (a mask), the 2e4 arguments of the [2^49, 2^50) vector, so that the top
    of the short reduction is weighed, not grazed."""
    rng = np.random.default_rng(12)
    x = np.concatenate([
        rng.uniform(-1, 1, 20000) * 10.0 ** rng.uniform(0, 300, 20000),
        rng.uniform(-1, 1, 20000) * 2.0 ** rng.uniform(28, 56, 20000),
        2.0 ** np.arange(0, 1024), -(2.0 ** np.arange(0, 1024)),
        2.0 ** 50 + np.arange(-64, 65) * 0.25,
        np.array([6381956970095103.0 * 2.0 ** 797, 5319372648326541416707072.0, 1e22, 2.343e22, -1.03e18]),
        rng.integers(1, 2 ** 22, 5000) * np.pi,                      # the doubles next to multiples of pi: sin ~ 1e-10
        rng.integers(1, 2 ** 22, 5000) * np.pi + np.pi / 2,          # ... and cos
    ])
    top = band_vector(49, 50)
    band = np.concatenate([np.zeros(x.size, bool), np.ones(top.size, bool)])
    x = np.concatenate([x, top])
    x.setflags(write=False)
    band.setflags(write=False)
    return x, band


@functools.lru_cache(maxsize=None)
def any_reference():
    """glibc's double sin / cos, which reduce every argument exactly."""
    x, _ = any_vector()
    return np.array([math.sin(v) for v in x]), np.array([math.cos(v) for v in x])


def any_bound():
    """Per-argument absolute bound: 1.5 * 2^-52, and the top band's measured figure on the band vector."""
    _, band = any_vector()
    return np.where(band, band_bound((49, 50)) * ULP53, 1.5 * 2.0 ** -52)


@functools.lru_cache(maxsize=None)
def switch_vector():
    x = 2.0 ** 50 + np.arange(-64, 65) * 0.25                        # 2^50 +- 16 in steps of 0.25: all exact doubles
    x = np.concatenate([x, -x])
    x.setflags(write=False)
    return x


def quadrant(x, r, q, sr, cr):
    """(sin x, cos x) from the long reduction's (r, q) and the kernels' (sin r, cos r), as sincos_any puts them together."""
    q = q.astype(np.int64)
    s = np.where(q & 1, cr, sr)
    c = np.where(q & 1, sr, cr)
    s = np.where(q & 2, -s, s)
    c = np.where((q + 1) & 2, -c, c)
    return np.where(x < 0, -s, s), c


# ---- the fp32 layer -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f32_vector():
    """2e6 floats in [-8, 8] and every float within 4 ulps of k pi/2, |k| <= 5 (as doubles holding float values)."""
    rng = np.random.default_rng(40)
    x = rng.uniform(-8, 8, 2_000_000).astype(np.float32)
    near = []
    for k in range(-5, 6):
        v = np.float32(k * (math.pi / 2))
        up = dn = v
        near.append(v)
        for _ in range(5):                       # the nearest float is within half an ulp: five steps cover four ulps
            up = np.nextafter(up, np.float32(np.inf), dtype=np.float32)
            dn = np.nextafter(dn, np.float32(-np.inf), dtype=np.float32)
            near += [up, dn]
    x = np.concatenate([x, np.array(near, dtype=np.float32)]).astype(np.float64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def f32_reference():
    x = f32_vector()
    return np.sin(x), np.cos(x)


SINCOS_F32_BOUND = 1.5               # units of 2^-24: the float emulation with the correct pi/2 split gives <= 1.24


@functools.lru_cache(maxsize=None)
def reduce_vector():
    """|x| <= 2e4 dense and log-uniform up to 2^48, 1e4 each."""
    rng = np.random.default_rng(41)
    x = np.concatenate([rng.uniform(-2.0e4, 2.0e4, 10000), 2.0 ** rng.uniform(-20, 48, 10000) * rng.choice([-1.0, 1.0], 10000)])
    x.setflags(write=False)
    return x


def ulp_f32(v):
    """The spacing of floats at |v| (v a Python float)."""
    return 2.0 ** (max(math.frexp(abs(v))[1] - 1, -126) - 23)


def check_reduce_2pi(x, r):
    """reduce_2pi_to_f32 against the reduction in mpmath: |r| <= float(pi) (1 + 2^-23) and
    |r - true| <= ulp_f32(true) / 2 + |x| 2^-100 + 2^-53, r and true compared modulo 2 pi.  Returns the worst excess
    (<= 0: all within) and the largest |r|."""
    import mpmath
    worst, at = -1.0, None
    with mpmath.workprec(240):
        twopi = 2 * mpmath.pi
        for xv, rv in zip(x.tolist(), r.tolist()):
            t = mpmath.mpf(xv)
            true = t - twopi * mpmath.nint(t / twopi)
            d = abs(rv - true)
            d = min(d, abs(d - twopi))
            tv = float(true)
            over = float(d - (mpmath.mpf(ulp_f32(tv)) / 2 + abs(t) * mpmath.mpf(2) ** -100 + mpmath.mpf(2) ** -53))
            if over > worst:
                worst, at = over, xv
    return worst, at, float(np.max(np.abs(r)))


R2PI_MAX = float(np.float32(math.pi)) * (1 + 2.0 ** -23)
# 1 / (2 pi) as the routine holds it is off by 9.84e-18: next to a half-integer of x / (2 pi) the nearest integer of the product is
# then the wrong neighbour once |x| is large, and r — still x modulo 2 pi — ends beyond pi by up to 2 pi |x| 9.84e-18
# (0.0174 at 2^48).  Harmless to the Newton loops (their sin / cos take [-8, 8]), but it is what the routine does.
INV_TWOPI_ERR = 9.84e-18


@functools.lru_cache(maxsize=None)
def reduce_edge_vector():
    """The doubles next to (k + 1/2) 2 pi for |x| from 2^20 to 2^48, where the choice of k is decided by the constant's error."""
    rng = np.random.default_rng(43)
    k = np.floor(2.0 ** rng.uniform(18, 45.3, 2000))
    x = ((k.astype(np.longdouble) + np.longdouble(0.5)) * (4 * PIO2_L)).astype(np.float64)
    x = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]) * rng.choice([-1.0, 1.0], 3 * x.size)
    assert np.abs(x).max() < 2.0 ** 48
    x.setflags(write=False)
    return x


def reduce_edge_range(x):
    """How far |r| may reach for these arguments: pi, the shift of the constant, and a float's rounding."""
    return math.pi + 2 * math.pi * np.abs(x) * INV_TWOPI_ERR + 2.0 ** -22


@functools.lru_cache(maxsize=None)
def div_vector():
    """n ~ N(0, 1) 10^[-6, 3], d in [0.01, 1.99], as floats (held in doubles)."""
    rng = np.random.default_rng(42)
    n = (rng.normal(0, 1, 2_000_000) * 10.0 ** rng.uniform(-6, 3, 2_000_000)).astype(np.float32)
    d = rng.uniform(0.01, 1.99, 2_000_000).astype(np.float32)
    n, d = n.astype(np.float64), d.astype(np.float64)
    n.setflags(write=False)
    d.setflags(write=False)
    return n, d


def div_pair_operands():
    """What debug_eval 34 / 35 and hm_div_f32x2 divide: (n, 3 n) by (d, 2 - d), formed in float."""
    n, d = div_vector()
    nf, df = n.astype(np.float32), d.astype(np.float32)
    return nf, np.float32(3) * nf, df, np.float32(2) - df


def div_ulps_off(got, nf, df):
    """(largest distance from the IEEE float quotient in float ulps of that quotient, share that is not bit-equal)."""
    ref = nf / df                                                     # float32 / float32: correctly rounded
    g = np.asarray(got, dtype=np.float64)
    off = np.abs(g - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    return float(off.max()), float(np.mean(g.astype(np.float32) != ref))


# ---- the Newton loops of the reduced-precision modes at the eccentricity clamp --------------------------------------------------
CLAMP_SWEEP_EPOCHS = 2048
CLAMP_SWEEP_POINTS = 1 << 16          # 2^27 solves


@functools.lru_cache(maxsize=None)
def clamp_sweep():
    """(fixed, table, parnames, theta): one planet at e = 0.99 (the clamp), one instrument; the epochs spread one period evenly
    and every point has its own ma0, so that M modulo 2 pi of the 2^27 solves covers [-pi, pi] densely."""
    from evidence_amd.data import EpochTable
    rng = np.random.default_rng(44)
    ne, b, period, epoch = CLAMP_SWEEP_EPOCHS, CLAMP_SWEEP_POINTS, 10.0, 51000.0
    t = epoch + period * (np.arange(ne) + rng.random(ne)) / ne
    table = EpochTable.from_arrays(["harps"], t, rng.normal(0.0, 3.0, ne), np.full(ne, 1.0), np.zeros(ne, dtype=np.int32))
    fixed = {"planet1_ecc": 0.99, "planet1_epoch": epoch}
    parnames = ["harps_jitter", "harps_offset", "planet1_k1", "planet1_ma0", "planet1_omega", "planet1_period"]
    theta = np.stack([np.full(b, 1.0), np.zeros(b), np.full(b, 5.0), rng.uniform(0, 2 * math.pi, b), rng.uniform(0, 2 * math.pi, b),
                      np.full(b, period)], axis=1)
    theta.setflags(write=False)
    return fixed, table, parnames, theta


# ---- the host build's exports: f(inputs..., n, outputs...) -----------------------------------------------------------------------
def host_call(lib, fn, ins, nout):
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
    outs = [np.empty(ins[0].size) for _ in range(nout)]
    getattr(lib, fn)(*[a.ctypes.data_as(dp) for a in ins], C.c_long(ins[0].size), *[o.ctypes.data_as(dp) for o in outs])
    return outs
