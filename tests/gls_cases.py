"""What the windowed tests of the GLS powers share (CPU and GPU): the cases (tables, rows, grids and the windows of
absolute frequency indices that are compared), the definition on a window in float64 and in long double with the summation order,
the phase order and a 1-ulp nudge of every sin and cos as knobs, delta of a window from those alone, a numpy emulation of the
arithmetic of weights_kernel and gls_kernel (csrc/rvll_gls.hip), and defects that can be switched on in the emulation.

The bound of a window is 8 delta of THAT window, row by row: delta grows with the phase (on the 51 Peg table from 1e-15 in the
first 512 frequencies to 3e-13 at f span = 16000), so one delta for a long grid would let an error of 1e-13 pass at the low
frequencies, 100 times the float64 noise there.  delta comes from the definition alone, never from the device.

The emulation is plain float64: where the kernels fuse a multiply and an add it rounds twice.  It stands in for the device on
a machine without one: it must lie within every window's bound, and every defect must take it out."""
import math
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import correlated_cases as cc
from evidence_amd.data import EpochTable
from evidence_amd.synthetic import make_workload

LD = cc.LD
FACTOR = 8.0                                # the bound of a window is FACTOR delta of that window (tests/test_gpu_periodogram.py's)
PARITY = cc.PARITY
TILE = 512                                  # kGlsFreqs: the frequencies of a workgroup
BLOCK, WAVE = 64, 64                        # kGlsBlock, kWave
PHASES = ("f_tau", "ftau", "tau_f")
ORDERS = ("pairwise", "sequential", "reversed")
NE_EDGES = (4, 5, 63, 64, 65, 255, 256, 257, 320, 513)
LONG_F = (1 << 18) + 3
LONG_WINDOWS = ((0, 512), (512, 512), (1024, 512), (11264, 512), (131072, 512), (262144, 3), (130816, 512))
EDGE_F = 1030
EDGE_WINDOWS = ((0, 512), (512, 512), (1024, 6))
CADENCE_F = 2304
CADENCE_WINDOWS = ((0, 512), (512, 512), (1792, 512), (2000, 256))
# 65 epochs 30 s apart span 64 steps, so f_k = (k + 1) / (8 span) times the step is (k + 1) / 512: a multiple of 1/2 at these nine
# indices (0.39 % of the grid), where every sine is 0 in exact arithmetic (and at the whole multiples every cosine 1): SS, CS and
# D are rounding residue there and the power is 0 / 0.  They are left out of every comparison; nothing else is.
CADENCE_SKIP = tuple(k for k in range(CADENCE_F) if (k + 1) % 256 == 0)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def peg51_table():
    from evidence_amd.config import read_config
    cfg = Path(__file__).resolve().parents[1] / "examples" / "51peg" / "config_51peg.py"
    _, datadict, _, _ = read_config(cfg, nplanets=1)
    return EpochTable.from_datadict(datadict)


def sinusoid_table(ne=100):
    """One instrument, 100 epochs over 200 days out of time order, a sinusoid of 50 at P = 7.3 d under noise of 1: the peak power
    of every row is above 0.9."""
    rng = np.random.default_rng(4100 + ne)
    t = 55000.25 + rng.uniform(0.0, 200.0, ne)
    vrad = 50.0 * np.cos(2.0 * np.pi * t / 7.3 + 0.4) + rng.normal(0.0, 1.0, ne) + 3.0
    return EpochTable.from_arrays(["a"], t, vrad, rng.uniform(0.8, 1.2, ne), np.zeros(ne, dtype=np.int32))


def two_svrad_table(ne=130):
    """Two instruments that alternate along time, listed instrument by instrument, with svrad of 0.3 and 30: the weights of the
    epochs span four decades."""
    rng = np.random.default_rng(4200 + ne)
    t = 55000.25 + np.cumsum(rng.uniform(0.02, 3.0, ne))
    inst = np.arange(ne) % 2
    order = np.argsort(inst, kind="stable")
    svrad = np.where(inst == 0, 0.3, 30.0)
    vrad = rng.normal(0.0, 4.0, ne) + rng.normal(0.0, 1.0, ne) * svrad
    return EpochTable.from_arrays(cc.INSTS, t[order], vrad[order], svrad[order], inst[order].astype(np.int32))


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def offsets_jitter_names(table):
    return [f"{i}_offset" for i in table.insts] + [f"{i}_jitter" for i in table.insts]


def offsets_jitter_rows(table, seed=0):
    """Five rows {name: [5]} of the offsets-and-jitter model on a table (five, so that the kernel's tile of 4 rows has a tail):
    offsets near the instrument's mean; an offset 30 scatters away (sum w r^2 - Y^2 cancels); jitter 0; jitter 50; a prior draw."""
    rng = np.random.default_rng(5000 + seed)
    inst_id = np.asarray(table.inst_id)
    out = {}
    for i, name in enumerate(table.insts):
        v = np.asarray(table.vrad)[inst_id == i]
        mean, std = float(v.mean()), float(v.std()) + 1.0
        out[f"{name}_offset"] = np.array([mean + 0.1, mean + 30.0 * std, mean - 0.3, mean + 0.2, mean + rng.uniform(-10.0, 10.0)])
        out[f"{name}_jitter"] = np.array([1.0, 1.0, 0.0, 50.0, rng.uniform(0.0, 5.0)])
    return out


def rows_theta(rows, parnames):
    return np.ascontiguousarray(np.stack([rows[name] for name in parnames], axis=1))


def offsets_jitter_residuals(table, rows):
    """(res, var) [5, Ne] of the rows by the definition's lines for a model without planets: res = vrad - offset of the epoch's
    instrument, var = svrad^2 + jitter^2."""
    inst_id = np.asarray(table.inst_id)
    n = len(next(iter(rows.values())))
    res, var = np.empty((n, inst_id.shape[0])), np.empty((n, inst_id.shape[0]))
    for i, name in enumerate(table.insts):
        idx = np.flatnonzero(inst_id == i)
        res[:, idx] = np.asarray(table.vrad)[idx][None, :] - rows[f"{name}_offset"][:, None]
        var[:, idx] = (np.asarray(table.svrad)[idx] ** 2)[None, :] + (rows[f"{name}_jitter"] ** 2)[:, None]
    return res, var


# ---- cases -------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    make: object                            # () -> EpochTable
    f0_spans: float = 0.125                 # f0 in units of 1 / span (df is 1 / (8 span) throughout)
    F: int = EDGE_F
    windows: tuple = EDGE_WINDOWS
    model: str = "offsets"                  # "offsets": the offsets-and-jitter model; "51peg" / "extras": test_gpu_periodogram's
    parity: bool = True                     # 8 delta of every window must be <= PARITY (Ne >= 63, no 3000-day gap)
    skip: tuple = ()                        # absolute indices left out of every comparison: the cadence table's aliases
    _table: object = field(default=None, repr=False)

    @property
    def table(self):
        if self._table is None:
            self._table = self.make()
        return self._table

    def grid(self):
        time = np.asarray(self.table.time, dtype=np.float64)
        span = float(time.max() - time.min())
        return self.f0_spans / span, 1.0 / (8.0 * span)

    def host_rows(self):
        """(time, res, var) without a device: the offsets-and-jitter rows on the case's table (for 51 Peg and extras too, whose
        device rows are prior draws of the models with their planets)."""
        rows = offsets_jitter_rows(self.table)
        res, var = offsets_jitter_residuals(self.table, rows)
        return np.array(self.table.time, dtype=np.float64), res, var


def _cases():
    out = [Case("51peg", peg51_table, F=LONG_F, windows=LONG_WINDOWS, model="51peg"),
           Case("extras", lambda: make_workload(3).table, F=LONG_F, windows=LONG_WINDOWS, model="extras")]
    for ne in NE_EDGES:
        out.append(Case(f"sorted{ne}", lambda ne=ne: cc.sorted_table(ne), parity=ne >= 63))
        out.append(Case(f"decreasing{ne}", lambda ne=ne: cc.decreasing_table(ne), parity=ne >= 63))
    for ne in (65, 257):
        # at its lowest frequencies the geometry of two clusters 3000 days apart is itself singular (the float64 definition is off
        # by up to 3e-9 there, which tests nothing): the grid starts at 96 / span
        out.append(Case(f"gap{ne}", lambda ne=ne: cc.make_table(ne), f0_spans=96.0, parity=False))
    out.append(Case("sinusoid", sinusoid_table))
    out.append(Case("two_svrad", two_svrad_table))
    out.append(Case("cadence65", lambda: cc.cadence_table(65), F=CADENCE_F, windows=CADENCE_WINDOWS, parity=False, skip=CADENCE_SKIP))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ---- the definition on a window ----------------------------------------------------------------------------------------------------
def _sum(x, order):
    """The sum over the last axis: numpy's pairwise sum, one running sum from the first term, or one from the last."""
    if order == "pairwise":
        return x.sum(axis=-1)
    if order == "sequential":
        return np.cumsum(x, axis=-1)[..., -1]
    if order == "reversed":
        return np.cumsum(x[..., ::-1], axis=-1)[..., -1]
    raise ValueError(f"unknown summation order {order!r}")


def _nudge(x, rng):
    up = rng.integers(0, 2, x.shape).astype(bool)
    return np.nextafter(x, np.where(up, np.inf, -np.inf).astype(x.dtype))


def window(time, res, var, f0, df, k0, nk, dtype=np.float64, phase="f_tau", order="pairwise", nudge=None, parts=False):
    """periodogram.gls_definition on the absolute indices k0 .. k0 + nk - 1 of the grid f0 + df k -> power [n, nk].  order names
    the summation (_sum); nudge is a seed: every sin and cos value moves by one ulp with a seeded random sign (libm's last bit, as
    OracleModel.conditioning has it).  At k0 = 0 with the defaults it is gls_definition bit for bit.  parts=True returns
    (power, rho) with rho = D / (CC SS), 1 minus the squared correlation of the cosine and sine columns."""
    time = np.asarray(time, dtype=dtype).reshape(-1)
    res, var = np.atleast_2d(np.asarray(res, dtype=dtype)), np.atleast_2d(np.asarray(var, dtype=dtype))
    two_pi = dtype(2.0) * (np.pi if dtype is np.float64 else np.arccos(dtype(-1.0)))
    tau = time - time.min()
    f = dtype(f0) + dtype(df) * np.arange(k0, k0 + nk, dtype=dtype)
    if phase == "f_tau":
        ph = (two_pi * f)[:, None] * tau[None, :]
    elif phase == "ftau":
        ph = two_pi * (f[:, None] * tau[None, :])
    elif phase == "tau_f":
        ph = (two_pi * tau)[None, :] * f[:, None]
    else:
        raise ValueError(f"unknown phase order {phase!r}")
    c, s = np.cos(ph), np.sin(ph)
    if nudge is not None:
        rng = np.random.default_rng(nudge)
        c, s = _nudge(c, rng), _nudge(s, rng)
    power = np.full((res.shape[0], nk), np.nan, dtype=dtype)
    rho = np.full((res.shape[0], nk), np.nan, dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(res.shape[0]):
            inv = dtype(1.0) / var[b]
            w = inv / _sum(inv, order)
            r = res[b]
            wr = w * r
            Y = _sum(wr, order)
            C, S = _sum(w * c, order), _sum(w * s, order)
            YY = _sum(wr * r, order) - Y * Y
            YC, YS = _sum(wr * c, order) - Y * C, _sum(wr * s, order) - Y * S
            CC, SS = _sum(w * c * c, order) - C * C, _sum(w * s * s, order) - S * S
            CS = _sum(w * c * s, order) - C * S
            D = CC * SS - CS * CS
            den = YY * D
            p = (SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS) / den
            power[b] = np.where(den > 0, p, np.nan)
            rho[b] = D / (CC * SS)
    return (power, rho) if parts else power


def evaluations():
    """The twelve float64 evaluations whose distance from long double is delta: 3 phase orders x 3 summation orders, and one
    nudged evaluation a phase order."""
    out = [dict(phase=p, order=o) for p in PHASES for o in ORDERS]
    return out + [dict(phase=p, order="pairwise", nudge=31 + i) for i, p in enumerate(PHASES)]


def kept(win, skip=()):
    """Which of the window's frequencies are compared: all but the case's skip list."""
    k0, nk = win
    return ~np.isin(np.arange(k0, k0 + nk), np.asarray(skip, dtype=np.int64))


def delta(data, win, skip=()):
    """(delta [n], wide [n, nk]) of the window (k0, nk) of data = (time, res, var, f0, df): wide is the long-double window and
    delta, row by row, the largest distance from it over the window's kept frequencies of the twelve float64 evaluations.  A
    power's bits depend on its own row alone, and a row whose sum w r^2 - Y^2 cancels has a delta 10 to 50 times its
    neighbours': a delta over all rows would lend that slack to every row.  The delta of the window as a whole is max(delta), so
    8 delta row by row is never wider than 8 delta of the window.  wide and the evaluations must be finite at every kept
    frequency: a NaN there is a fault of the case, not a figure."""
    time, res, var, f0, df = data
    k0, nk = win
    keep = kept(win, skip)
    wide = window(time, res, var, f0, df, k0, nk, dtype=LD)
    assert np.all(np.isfinite(wide[:, keep])), ("the long-double window has a NaN at a kept frequency", win)
    d = np.zeros(wide.shape[0])
    for kw in evaluations():
        e = window(time, res, var, f0, df, k0, nk, **kw)
        assert np.all(np.isfinite(e[:, keep])), ("a float64 evaluation is NaN at a kept frequency", win, kw)
        d = np.maximum(d, np.max(np.abs(e[:, keep] - wide[:, keep]), axis=1).astype(np.float64))
    return d, wide


def errors(power, wide, win, skip=()):
    """The largest |power - wide| of every row over the window's kept frequencies [n] (inf where power is not finite there)."""
    keep = kept(win, skip)
    err = np.abs(np.asarray(power, dtype=np.float64)[:, keep].astype(LD) - wide[:, keep]).astype(np.float64)
    return np.max(np.where(np.isfinite(err), err, np.inf), axis=1)


def ratio(power, wide, d, win, skip=()):
    """(the largest error / delta of a row, the largest error / the window's delta): the first is held to FACTOR."""
    err = errors(power, wide, win, skip)
    return float(np.max(err / d)), float(np.max(err) / np.max(d))


def references(case, data):
    """[(window, delta, wide)] of a case's windows on data = (time, res, var, f0, df): computed once by the caller and left
    unchanged."""
    return [(win,) + delta(data, win, case.skip) for win in case.windows]


def rho_long_double(data, win):
    """rho = D / (CC SS) [n, nk] of a window in long double."""
    time, res, var, f0, df = data
    return window(time, res, var, f0, df, win[0], win[1], dtype=LD, parts=True)[1]


# ---- the kernels' arithmetic in numpy ----------------------------------------------------------------------------------------------
TWO_PI = 6.283185307179586476925286766559       # kGlsTwoPi
DEFECTS = ("neighbour_row", "df_float32", "short_polynomials")


def _wave_sum(v):
    """gls_wave_sum: the xor tree over 64 lanes; every lane ends with the same sum."""
    lanes = np.arange(WAVE)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m]
    return v[..., 0]


def _lanes(x):
    """A lane's running sum over the epochs lane, lane + 64, ... in order -> [n, 64]."""
    n, ne = x.shape
    pad = np.zeros((n, -(-ne // WAVE) * WAVE))
    pad[:, :ne] = x
    out = np.zeros((n, WAVE))
    for k in range(pad.shape[1] // WAVE):
        out = out + pad[:, k * WAVE:(k + 1) * WAVE]
    return out


def emulate_weights(res, var):
    """weights_kernel: (w, wr [n, Ne], W, Y, YY [n]).  (The kernel's yy = fma(wri, r, yy) rounds once; here twice.)"""
    inv = 1.0 / var
    total = _wave_sum(_lanes(inv))
    w = inv / total[:, None]
    wr = w * res
    W, Y, yy = _wave_sum(_lanes(w)), _wave_sum(_lanes(wr)), _wave_sum(_lanes(wr * res))
    return w, wr, W, Y, yy - Y * Y


def _sincos(ph, defect):
    """sin and cos of the phases.  short_polynomials: after the reduction to |r| <= pi / 4 the sine series loses its r^15 term and
    the cosine series its r^14 term (at most 2e-14 and 4e-13)."""
    if defect != "short_polynomials":
        return np.sin(ph), np.cos(ph)
    half_pi = np.arccos(LD(-1.0)) / 2
    q = np.rint(ph / (np.pi / 2.0))
    r = (ph.astype(LD) - q.astype(LD) * half_pi).astype(np.float64)
    sr = np.sin(r) + r ** 15 / math.factorial(15)
    cr = np.cos(r) + r ** 14 / math.factorial(14)
    quad = q.astype(np.int64) & 3
    s = np.choose(quad, [sr, cr, -sr, -cr])
    c = np.choose(quad, [cr, -sr, -cr, sr])
    return s, c


def emulate(time, res, var, f0, df, k0, nk, defect=None):
    """gls_kernel on the absolute indices k0 .. k0 + nk - 1 (k0 even) of rows res, var [n, Ne] at the table's epochs `time`, in
    table order -> power [n, nk] float64.  One sincos at every even k and one rotation to k + 1, the terms of 64 consecutive
    epochs added in table order and the blocks' sums then, W, Y, YY by emulate_weights, the powers by the kernel's lines with the
    definition's guard.  defect switches one of DEFECTS on:
      neighbour_row      the last epoch of every block takes the next row's w r;
      df_float32         the rotation to the odd k is by 2 pi float32(df) tau;
      short_polynomials  _sincos."""
    assert k0 % 2 == 0 and (defect is None or defect in DEFECTS)
    time = np.asarray(time, dtype=np.float64)
    res, var = np.atleast_2d(res), np.atleast_2d(var)
    n, ne = res.shape
    w, wr, W, Y, YY = emulate_weights(res, var)
    tau = time - time.min()
    ke = np.arange(k0, k0 + nk, 2)
    om = TWO_PI * (f0 + df * ke.astype(np.float64))
    dom = TWO_PI * (float(np.float32(df)) if defect == "df_float32" else df)
    s0, c0 = _sincos(om[:, None] * tau[None, :], defect)                  # [K / 2, Ne]
    sd, cd = _sincos(dom * tau, defect)
    c1, s1 = c0 * cd - s0 * sd, s0 * cd + c0 * sd
    K = 2 * ke.shape[0]
    c, s = np.empty((K, ne)), np.empty((K, ne))
    c[0::2], c[1::2], s[0::2], s[1::2] = c0, c1, s0, s1
    c2, cs = c * c - s * s, c * s
    tot = np.zeros((6, n, K))
    for i0 in range(0, ne, BLOCK):
        i1 = min(i0 + BLOCK, ne)
        acc = np.zeros((6, n, K))
        for i in range(i0, i1):
            wv, wrv = w[:, i, None], wr[:, i, None]
            if defect == "neighbour_row" and i == i1 - 1:
                wrv = np.roll(wr[:, i], -1)[:, None]
            for q, (a, col) in enumerate(((wv, c), (wv, s), (wv, c2), (wv, cs), (wrv, c), (wrv, s))):
                acc[q] = a * col[None, :, i] + acc[q]
        tot = tot + acc
    hw, y, yy = 0.5 * W[:, None], Y[:, None], YY[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        C, S, A = tot[0], tot[1], 0.5 * tot[2]
        CC, SS, CS = (hw + A) - C * C, (hw - A) - S * S, tot[3] - C * S
        YC, YS = tot[4] - y * C, tot[5] - y * S
        D = CC * SS - CS * CS
        num = SS * YC * YC + CC * YS * YS - 2.0 * CS * YC * YS
        den = yy * D
        p = np.where(den > 0.0, num / den, np.nan)
    return p[:, :nk]
