"""A float32 restatement of the reduced-precision log-L modes (precision="mixed" / "fp32") in plain numpy, and the seeded edge
shapes they are held to: shared by tests/test_reduced_cases_host.py (the emulation against the fp64 oracle: is it the modes'
class, are the inputs what the GPU tests need?) and tests/test_gpu_reduced_shapes.py (the device against the oracle, bounded
by the emulation's own distance from it).

emulate() follows evidence_amd/csrc/rvll_tile.h operation by operation wherever a float appears (the lines are cited where
they are restated), the wave-wide stop rule of eval_item_pair included where it is given the launch geometry (an item that
has met the stop rule takes the steps its wave still takes: closer to its root, and at a coarse tol FARTHER from a reference that
stops each solve by itself — 1e-5 of log-L at tol = 1e-2).  What it does not model: the device's sincos_f32 and div_f32 (numpy's float sin / cos / division stand in: within half an ulp where the device's are within 1.24 and 1 ulp), and the
order of the fp64 sums of a point (lane-strided and a shuffle tree on the device, numpy's pairwise sum here: 1e-16)."""
from types import SimpleNamespace

import numpy as np

from evidence_amd import _abi
from evidence_amd.layout import compile_layout
from test_gpu_loglike import _synthetic_case

f32 = np.float32
K_F32_STEPS = 16          # rvll_math.h kF32Steps: a float solve not settled by then is done in double
K_SAFE_STEPS = 8          # rvll_math.h kSafeSteps: more steps than this is RVLL_FLAG_WANDERED
F32_MIN_TOL = 2.0 ** -22  # rvll_math.h kF32MinTol: below this tol every solve is done in double
LONG_SOLVE_ECC = 0.9     # rvll_math.h kLongSolveEcc: the CU-wide form starts its rounds at such a point (tile_decode)
TWO_PI = 6.283185307179586
PRECISIONS = ("mixed", "fp32")


def sincos_numpy(x):
    return np.sin(x), np.cos(x)


def sincos_nudged(direction):
    """numpy's float sin / cos moved one float ulp up (+1) or down (-1): the conditioning idiom of oracle.OracleModel, in float."""
    to = f32(np.inf * direction)
    return lambda x: (np.nextafter(np.sin(x), to), np.nextafter(np.cos(x), to))


def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in a double, the sum is rounded there and again to float."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def reduce_2pi_to_f32(M):
    """rvll_math.h reduce_2pi_to_f32: M to [-pi, pi] in fp64, then one rounding to float (the fp64 remainder is good to 1e-12 at
    |M| ~ 1e4, far below a float ulp)."""
    k = np.rint(M * 1.59154943091895335769e-01)
    return ((M - k * 6.28318530717958623200e+00) - k * 2.44929359829470641435e-16).astype(f32)


def newton_f32(sincos, Mf, ecf, tolf, cap):
    """The float Newton rule of both item paths (rvll_tile.h:502-512, :672-684) per item: start E = Mf, at least one step, stop
    when abs(dE) <= tol (NaN-safe), at most `cap` steps.  Flat float32 arrays in; (E, dE of the last step, sin and cos at the
    iterate BEFORE the last step, step count, settled) out."""
    n = Mf.size
    E, dE = Mf.copy(), np.zeros(n, f32)
    s, c = np.zeros(n, f32), np.zeros(n, f32)
    steps, live = np.zeros(n, np.int32), np.arange(n)
    one = f32(1)
    for _ in range(cap):
        El, el, Ml = E[live], ecf[live], Mf[live]
        sl, cl = sincos(El)
        f = El - el * sl - Ml                       # :506 / :674 (no contraction: the library is built with -ffp-contract=off)
        fp = one - el * cl                          # :507 / :675
        En = El - f / fp                            # :508 / :676
        d = En - El
        E[live], dE[live], s[live], c[live] = En, d, sl, cl
        steps[live] += 1
        live = live[~(np.abs(d) <= tolf)]
        if live.size == 0:
            break
    settled = np.ones(n, bool)
    settled[live] = False
    return E, dE, s, c, steps, settled


def newton_f32_waves(sincos, Mf, ecf, tolf, gid, cap):
    """newton_f32 under the wave-wide stop rule of eval_item_pair (rvll_tile.h:680-684): the items of one wave, both of every
    lane — gid[i] numbers the wave item i is solved in (pair_waves) — step together until every one of them has met the stop
    rule at the same step, `cap` steps at the most.  An item is settled if its LAST step met the rule (:687)."""
    n = Mf.size
    E, dE = Mf.copy(), np.zeros(n, f32)
    s, c = np.zeros(n, f32), np.zeros(n, f32)
    steps, live = np.zeros(n, np.int32), np.arange(n)
    one, going = f32(1), np.zeros(int(gid.max()) + 1, bool)
    for _ in range(cap):
        El, el, Ml = E[live], ecf[live], Mf[live]
        sl, cl = sincos(El)
        En = El - (El - el * sl - Ml) / (one - el * cl)
        d = En - El
        E[live], dE[live], s[live], c[live] = En, d, sl, cl
        steps[live] += 1
        going[:] = False
        going[gid[live][~(np.abs(d) <= tolf)]] = True
        live = live[going[gid[live]]]
        if live.size == 0:
            break
    return E, dE, s, c, steps, np.abs(dE) <= tolf


def pair_waves(rows, n_epochs, form, pb, start_rounds=None, window=4096):
    """Which items the pair path (itmax > 16) solves in one wave, as loglike_tile deals them (rvll_tile.h:1186-1258): a wave
    number per flattened (row, epoch) item, and (item, wave) of the copies that ride along — a lane of the CU-wide form beyond the
    tile's last item is pointed at item (0, 0) of the tile (:1227) and takes part in its wave's stop test.
      "tile": tiles of pb rows, LDS windows of `window` items cut at point-local positions (:1183-1187, rvll_api.hip:171-172);
              in a window thread t of 256 takes items t + 512 k and t + 256 + 512 k (:1247-1248), 64 threads a wave
      "cu":   one window; tickets are drawn in twos (:1196), ticket k is wave round (k + r0) mod rounds (:1206-1207, :1218-1219)
              with r0 the tile's start round (start_rounds, tile_decode :857-859)"""
    gid = np.empty(rows * n_epochs, np.int64)
    ghost_item, ghost_gid, g = [], [], 0
    for t, p0 in enumerate(range(0, rows, pb)):
        n, first = min(pb, rows - p0) * n_epochs, p0 * n_epochs
        if form == "tile":
            ch = (min(window, max(256, pb * n_epochs)) + 1) & ~1
            wpts, base = (ch // n_epochs if n_epochs <= ch else 0), 0
            while base < n:
                cend = min(base + wpts * n_epochs, n) if wpts else min(base + ch, (base // n_epochs + 1) * n_epochs)
                rel = np.arange(cend - base)
                gid[first + base:first + cend] = g + (rel // 512) * 4 + (rel % 256) // 64
                g += -(-(cend - base) // 512) * 4
                base = cend
        else:
            rounds = -(-n // 64)
            r0 = int(start_rounds[t]) if start_rounds is not None else 0
            ticket = (np.arange(n) // 64 - r0) % rounds
            gid[first:first + n] = g + ticket // 2
            if n % 64:
                ghost_item.append(first)
                ghost_gid.append(g + ((rounds - 1 - r0) % rounds) // 2)
            g += -(-rounds // 2)
    return gid, np.array(ghost_item, np.int64), np.array(ghost_gid, np.int64)


def newton_f64(M, ec, tol, cap):
    """The solve a float iteration is handed over to (rvll_tile.h:517-528, pair_solve_f64 :626-637): the reference's rule from
    E = M in fp64 — solver_cases.newton_counts is the same rule and returns these counts.  (E, step count) per item."""
    E, steps, live = M.copy(), np.zeros(M.size, np.int32), np.arange(M.size)
    for _ in range(cap):
        El = E[live]
        f = El - ec[live] * np.sin(El) - M[live]
        En = El - f / (1 - ec[live] * np.cos(El))
        d = En - El
        E[live] = En
        steps[live] += 1
        live = live[np.abs(d) > tol]
        if live.size == 0:
            break
    return E, steps


def layout_of(case, tol=None, itmax=None):
    """The layout GpuRVModel compiles for the case (linear terms included), for the oracle and the emulation."""
    lay = compile_layout(case.parnames, case.fixed, case.table.insts, list(getattr(case, "linpar", None) or {}))
    if tol is not None:
        lay.tol = float(tol)
    if itmax is not None:
        lay.itmax = int(itmax)
    return lay


def linpar_series(case, lay):
    return np.stack([case.linpar[k] for k in lay.linpar_names]) if lay.linpar_names else None


def _slot(s, theta):
    return theta[:, s.index] if s.index >= 0 else np.full(theta.shape[0], s.value)


def decode(lay, theta):
    """decode_planet (rvll_tile.h:822-878) in fp64, per (row, planet): 2 pi / P, epoch, ma0, the clamped eccentricity,
    A = K cos w, Bq = K sqrt(1 - e^2) sin w, C0 = K e cos w (the unclamped e, as the reference has it); invalid[rows]."""
    n, npl = theta.shape[0], len(lay.planets)
    out = {k: np.zeros((n, npl)) for k in ("w", "epoch", "ma0", "ec", "A", "Bq", "C0")}
    invalid = np.zeros(n, bool)
    for i, d in enumerate(lay.planets):
        kraw, praw = _slot(d.k, theta), _slot(d.p, theta)
        K = np.exp(kraw) if d.k_kind == _abi.K_LOGK1 else kraw
        Pd = np.exp(praw) if d.p_kind == _abi.P_LOGPERIOD else praw
        e1, e2 = _slot(d.e1, theta), _slot(d.e2, theta)
        if d.ecc_kind == _abi.ECC_SECOS_SESIN:
            ecc, omega = e1 * e1 + e2 * e2, np.arctan2(e2, e1)
            invalid |= ecc > 1
        elif d.ecc_kind == _abi.ECC_ECOS_ESIN:
            ecc, omega = np.sqrt(e1 * e1 + e2 * e2), np.arctan2(e2, e1)
            invalid |= ecc > 1
        else:
            ecc, omega = e1, e2
        anom = _slot(d.anom, theta)
        ec = np.where(ecc > 0.99, 0.99, ecc)                                    # :851, trueanomaly.c:11-12
        so, co = np.sin(omega), np.cos(omega)
        out["w"][:, i] = TWO_PI / Pd
        out["epoch"][:, i] = _slot(d.epoch, theta)
        out["ma0"][:, i] = anom - omega if d.anom_kind == _abi.ANOM_ML0 else anom
        out["ec"][:, i] = ec
        out["A"][:, i] = K * co
        out["Bq"][:, i] = K * np.sqrt((1. - ec) * (1. + ec)) * so
        out["C0"][:, i] = K * (ecc * co)
    return out, invalid


def _planet_term(sincos, M, ec, A, Bq, C0, tol, itmax, waves=None):
    """One planet's term K (cos(nu + w) + e cos w) at every (row, epoch) [rows, Ne], the items handed to the double solver and
    the items whose solve ran out of steps.  ec, A, Bq, C0: [rows, 1]."""
    shape = M.shape
    bc = lambda v: np.broadcast_to(v, shape).ravel()
    Mr, ecr, Ar, Br, Cr = M.ravel(), bc(ec), bc(A), bc(Bq), bc(C0)
    Mf, ecf, tolf = reduce_2pi_to_f32(Mr), ecr.astype(f32), f32(tol)            # :500-501 / :667-668, :655
    pairs = itmax > K_F32_STEPS                                                 # :1185
    if pairs and waves is not None:
        gid, ghost_item, ghost_gid = waves                  # the copies that ride along are solved too, and dropped
        src = np.concatenate([np.arange(Mf.size), ghost_item])
        E, dE, s, c, steps, settled = (v[:Mf.size] for v in newton_f32_waves(sincos, Mf[src], ecf[src], tolf,
                                                                              np.concatenate([gid, ghost_gid]), K_F32_STEPS))
    else:
        E, dE, s, c, steps, settled = newton_f32(sincos, Mf, ecf, tolf, min(itmax, K_F32_STEPS))
    astray = ~(np.abs(E - Mf) <= f32(1) + tolf)                                 # :278 f32_astray
    # :513 / :687: not settled after the float steps, or settled where no root can be -> in double from its start; the single-item
    # path (itmax <= 16) only where the float loop stopped short of itmax: at itmax the item is a failed solve (:541)
    handed = (~settled | astray) & (pairs | (steps < itmax))
    # ... and every solve where tol is below what a float step can show (rvll_math.h kF32MinTol: a step under half an ulp of E
    # rounds to 0 and passes any stop test)
    handed |= tol < F32_MIN_TOL
    failed = ~handed & ~pairs & (steps >= itmax)
    if pairs and tol <= 1e-3:
        # :690-693: (s, c) are at the iterate before the last step; rotated by that step, h^3 / 6 dropped
        hh = f32(0.5) * dE * dE
        s, c = _fma(c, dE, _fma(-s, hh, s)), _fma(-s, dE, _fma(-c, hh, c))
    else:
        s, c = sincos(E)                                                        # :536 / :695: evaluated again at the iterate
    den = _fma(-ecf, c, np.ones_like(c))                                        # :537 / :697
    num = _fma(Ar.astype(f32), c - ecf, -(Br.astype(f32) * s))                  # :538 / :699
    rv = (num / den + Cr.astype(f32)).astype(np.float64)                        # :539 / :700-701
    if handed.any():
        h = np.flatnonzero(handed)
        Ed, n64 = newton_f64(Mr[h], ecr[h], tol, itmax)
        cd, sd = np.cos(Ed), np.sin(Ed)
        rv[h] = (Ar[h] * (cd - ecr[h]) - Br[h] * sd) / (1. - ecr[h] * cd) + Cr[h]      # :531-532 / :640-641
        failed[h] = n64 >= itmax                                                # :530 / :639
    rv, failed = rv.reshape(shape), failed.reshape(shape)
    # the reference leaves nu = 0 from a planet's first failing epoch on (trueanomaly.c:32-33): the tile's redo pass (3b,
    # rvll_tile.h:1278-1297; eval_item :348-351) puts A + C0 there
    first = np.where(failed.any(axis=1), failed.argmax(axis=1), shape[1])
    marked = np.arange(shape[1])[None, :] >= first[:, None]
    rv = np.where(marked, A + C0, rv)
    return rv, handed.reshape(shape), first


def emulate(case, precision, tol=1e-4, itmax=10000, sincos=sincos_numpy, info=None, geometry=None):
    """log-L per row as the reduced-precision branch of eval_item (itmax <= 16), or eval_item_pair / pair_tail (itmax > 16),
    computes it.  geometry: None — every item stops by itself — or (form, points per tile): the items of the pair path stop
    wave by wave, as that launch deals them (pair_waves).  info: a dict that receives `handed` (items solved in double), `first` ([rows, planets] first failing epoch,
    the epoch count where none) and `flags` (RVLL_FLAG_NONCONVERGED per row)."""
    assert precision in PRECISIONS
    lay = layout_of(case)
    theta = np.ascontiguousarray(case.theta, dtype=np.float64)
    tb = case.table
    t, y, s2, inst = tb.time, tb.vrad, tb.svrad * tb.svrad, tb.inst_id
    n, ne = theta.shape[0], t.size
    P, invalid = decode(lay, theta)
    off = np.stack([_slot(i.offset, theta) for i in lay.insts], axis=1)
    jit = np.stack([_slot(i.jitter, theta) for i in lay.insts], axis=1) if lay.has_jitter else np.zeros_like(off)
    rvm = 0. + off[:, inst]                                                     # :327 / :652, rvmodel:187
    var = s2[None, :] + (jit * jit)[:, inst]                                    # :328 / :653
    ksum = np.zeros((n, ne))
    handed, firsts = 0, np.full((n, max(1, len(lay.planets))), ne)
    waves = None
    if geometry is not None and itmax > K_F32_STEPS and lay.planets:
        form, pb = geometry
        waves = pair_waves(n, ne, form, pb, wrap_start_rounds(case, pb) if form == "cu" else None)
    for ip in range(len(lay.planets)):
        col = lambda k: P[k][:, ip:ip + 1]
        M = col("w") * (t[None, :] - col("epoch")) + col("ma0")                 # :499 / :665, rvmodel:459, in fp64
        rv, h, first = _planet_term(sincos, M, col("ec"), col("A"), col("Bq"), col("C0"), tol, itmax, waves)
        ksum = ksum + rv                                                        # :549 / :718, in planet order
        handed += int(h.sum())
        firsts[:, ip] = first
    rvm = rvm + ksum                                                            # :551 / :721
    if lay.has_drift:                                                           # :555-560 / :604-609
        d = [_slot(sl, theta)[:, None] for sl in lay.drift]
        tref = np.full((n, 1), t[0]) if lay.tref_from_data else _slot(lay.tref, theta)[:, None]
        tt = (t[None, :] - tref) * (1.0 / 365.25)
        t2 = tt * tt
        rvm = rvm + (d[0] * tt + d[1] * t2 + d[2] * (t2 * tt) + d[3] * (t2 * t2))
    series = linpar_series(case, lay)
    for k, sl in enumerate(lay.linpar):                                         # :561-562 / :610-611
        rvm = rvm + _slot(sl, theta)[:, None] * series[k][None, :]
    res = y[None, :] - rvm                                                      # :575 / :613
    if precision == "fp32":
        rf, vf = res.astype(f32), var.astype(f32)                               # :586-587 / :615-616
        item = (rf * rf / (f32(2) * vf)).astype(np.float64)
    else:
        item = res * res / (2 * var)                                            # :589 / :618
    # tile_logdet (:976-997, logdet_finish :962-974) is the same code in every precision: sum_j ln sqrt(var_j) in fp64, as the
    # logarithm of a (mantissa product, exponent sum); a.cte (rvll_api.hip:414) - acc (tile_point_result :1076)
    acc = 0.5 * np.log(var).sum(axis=1) + item.sum(axis=1)
    out = -0.5 * ne * np.log(2 * np.pi) - acc
    if len(lay.planets) > 0:
        out = np.where(invalid, -1e30, out)
    if info is not None:
        info["handed"] = handed
        info["first"] = firsts[:, :len(lay.planets)]
        info["flags"] = np.where((firsts < ne).any(axis=1), _abi.FLAG_NONCONVERGED, 0).astype(np.int32)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------

def _case(name, n_epochs, nplanets, ninst, drift, nlin, rows, form, pb=0, runs=((1e-4, 10000),), seed=0, ecc_top=None):
    """A seeded model of test_gpu_loglike._synthetic_case (eccentricities 0 .. 0.8: nothing wanders) with the geometry it is to
    be run at: form "tile" at `pb` points per block, or "cu" (the host sizes the tile from the batch: cu_geometry).  runs: the
    (tol, itmax) pairs.  ecc_top: planet 1 of every fifth row is put at this eccentricity (>= 0.9: the CU-wide form then starts
    its rounds at that point's round and wraps)."""
    rng = np.random.default_rng(7919 * n_epochs + 131 * nplanets + 17 * ninst + 3 * nlin + int(drift) + 1000003 * seed)
    table, free, fixed, ranges, linpar = _synthetic_case(rng, n_epochs, nplanets, ninst, drift, nlin, False)
    theta = np.stack([rng.uniform(*ranges[nm], rows) for nm in free], axis=1)
    if ecc_top is not None:
        theta[2::5, free.index("planet1_ecc")] = ecc_top
    return SimpleNamespace(name=name, table=table, parnames=list(free), fixed=dict(fixed), theta=np.ascontiguousarray(theta),
                           linpar=linpar, n_epochs=n_epochs, nplanets=nplanets, form=form, pb=pb, runs=tuple(runs),
                           wraps=ecc_top is not None)


BOTH = ((1e-4, 10000), (1e-4, 16))        # item pairs, and the single-item float loop
PAIRS = ((1e-4, 10000),)


def cases():
    """Every case has 256 rows or more (the maximum over rows is then a stable statistic)."""
    out = [
        # ---- 256-thread tiles: the pair is item i and item i + 256; items = n_epochs * pb
        #     name            Ne  Np Ni drift nlin rows form   pb
        _case("t1",            1, 1, 1, False, 0, 256, "tile", 1),
        _case("t63",          63, 8, 5, True,  3, 256, "tile", 1, BOTH),
        _case("t64",          64, 2, 2, False, 0, 256, "tile", 1, BOTH),
        _case("t65",          65, 3, 1, False, 1, 256, "tile", 1, BOTH),
        _case("t255",         17, 5, 2, False, 0, 256, "tile", 15),
        _case("t256",         64, 0, 2, True,  0, 256, "tile", 4),
        _case("t257",        257, 1, 3, True,  0, 256, "tile", 1, BOTH),
        _case("t300",        100, 3, 2, False, 0, 257, "tile", 3, BOTH),
        _case("t511",         73, 2, 1, False, 3, 259, "tile", 7),
        _case("t512",        128, 5, 1, False, 0, 256, "tile", 4),
        _case("t513",        171, 1, 4, False, 0, 256, "tile", 3),
        _case("t1000",       200, 2, 2, True,  1, 256, "tile", 5, BOTH),
        # ---- LDS windows of 4096 items: a second window of one item; a ragged second; a third
        _case("w4097_pb1",  4097, 1, 1, False, 0, 256, "tile", 1),
        _case("w4097_pb2",  4097, 1, 1, False, 0, 256, "tile", 2),
        _case("w4500_pb1",  4500, 2, 2, False, 0, 256, "tile", 1, BOTH),
        _case("w4500_pb2",  4500, 2, 2, False, 0, 256, "tile", 2, BOTH),
        _case("w8492_pb1",  8492, 1, 2, True,  0, 256, "tile", 1),
        _case("w8492_pb2",  8492, 1, 2, True,  0, 256, "tile", 2),
        # ---- tol off its default: a fresh sin / cos instead of the rotation; every solve handed to the double solver
        _case("t65_tols",     65, 3, 1, False, 1, 256, "tile", 1, ((1e-2, 10000), (1e-9, 10000))),
        _case("t300_tols",   100, 3, 2, False, 0, 257, "tile", 3, ((1e-2, 10000), (1e-9, 10000))),
        _case("c300_tols",   100, 3, 2, False, 0, 768, "cu", 0, ((1e-2, 10000), (1e-9, 10000))),
        # ---- the CU-wide form: the same models, rows chosen for the tile the host then cuts (cu_geometry; 256 CUs: up to 256
        # rows one point a tile, 257 .. 512 two, 513 .. 768 three)
        _case("c1",            1, 1, 1, False, 0, 256, "cu"),                 # 1 round, ragged
        _case("c63",          63, 8, 5, True,  3, 256, "cu", 0, BOTH),        # 1 round, ragged
        _case("c64",          64, 2, 2, False, 0, 256, "cu", 0, BOTH),        # 1 round, full
        _case("c65",          65, 3, 1, False, 1, 256, "cu", 0, BOTH),        # 2 rounds, ragged
        _case("c128",         64, 2, 2, False, 0, 512, "cu"),                 # 2 rounds, full (2 points)
        _case("c171",        171, 1, 4, False, 0, 256, "cu"),                 # 3 rounds, ragged
        _case("c192",         64, 0, 2, True,  0, 768, "cu"),                 # 3 rounds, full (3 points)
        _case("c200",        200, 2, 2, True,  1, 256, "cu", 0, BOTH),        # 4 rounds, ragged
        _case("c256",        128, 5, 1, False, 0, 512, "cu"),                 # 4 rounds, full (2 points)
        _case("c257",        257, 1, 3, True,  0, 256, "cu", 0, BOTH),        # 5 rounds, ragged
        _case("c300",        100, 3, 2, False, 0, 768, "cu", 0, BOTH),        # 5 rounds, ragged (3 points)
        _case("c300_wrap",   100, 3, 2, False, 0, 768, "cu", 0, PAIRS, ecc_top=0.9),     # ... starting at round 1 or 3: wraps
        _case("c146_wrap",    73, 2, 1, False, 3, 512, "cu", 0, PAIRS, ecc_top=0.9),     # 3 rounds, starting at round 1: wraps
        _case("c4500",      4500, 2, 2, False, 0, 256, "cu", 0, BOTH),        # 71 rounds, ragged
    ]
    assert len({c.name for c in out}) == len(out) and all(c.theta.shape[0] >= 256 for c in out)
    return out


def runs(case_list=None):
    """(case, tol, itmax) of every run of every case."""
    return [(c, tol, itmax) for c in (cases() if case_list is None else case_list) for tol, itmax in c.runs]


def run_id(case, tol, itmax):
    return f"{case.name}-tol{tol:g}-itmax{itmax}"


def cu_geometry(rows, n_epochs, n_cu=256):
    """Points per tile of the forced CU-wide form as rvll_api.hip choose_cu_form sizes it while one tile of
    ceil(rows / CUs) points fits the LDS budget (these cases: three points of 100 epochs at the most), wave rounds of a full
    tile, and whether the last round is ragged."""
    pb = -(-rows // min(n_cu, rows))
    assert pb <= 128
    items = pb * n_epochs
    return pb, -(-items // 64), items % 64 != 0


def wrap_start_rounds(case, pb):
    """The round the CU-wide form starts at, per tile (tile_decode, rvll_tile.h:857-859: the round the most eccentric point at or
    above kLongSolveEcc begins in; 0 where the tile has none)."""
    i = 0 if case.nplanets and "planet1_ecc" in case.parnames else None
    out = []
    for p0 in range(0, case.theta.shape[0], pb):
        r0 = 0
        if i is not None:
            best = -1
            for pl in range(min(pb, case.theta.shape[0] - p0)):
                e = max(min(case.theta[p0 + pl, case.parnames.index(f"planet{k}_ecc")], 0.99) for k in range(1, case.nplanets + 1))
                if e >= LONG_SOLVE_ECC:
                    key = (int((e - LONG_SOLVE_ECC) * 340.), (pl * case.table.time.size) >> 6)
                    best = max(best, key[0] * 1024 + min(key[1], 1023))
            r0 = best % 1024 if best >= 0 else 0
        out.append(r0)
    return np.array(out)


# ---- shared figures ----------------------------------------------------------------------------------------------------------

def oracle_of(case, tol=1e-4, itmax=10000):
    """(log-L, flags) of the fp64 oracle at the case's rows."""
    from oracle.oracle import OracleModel
    lay = layout_of(case, tol, itmax)
    return OracleModel(lay, case.table, linpar_series(case, lay)).loglike(case.theta, nthreads=8, return_flags=True)


def rel_err(a, b):
    import golden
    return golden.rel_err(a, b)


def fp64_term(case):
    """What the fp64 operations the emulation does not restate can move log-L by, relative: the order of a point's sums (pairwise
    here, lane-strided and through a shuffle tree on the device: one rounding of 2^-53 per term) and, per planet term of an item
    formed in double, sin, cos and the quotient at up to 1.24 ulp where numpy's are within half (four roundings) — taken as if
    they all added up.  1e-14 .. 5e-12 next to yardsticks near 1e-7; it is all there is where a mode has no float operation
    (mixed without planets, or with every solve handed to the double solver: Y ~ 5e-16)."""
    return case.table.time.size * (1 + 4 * case.nplanets) * 2.0 ** -53


def bound(case, y):
    """The device's bound against the oracle: four times the emulation's own distance from it (the margin: sincos_f32 is good to
    1.24 * 2^-24 where numpy's float sin / cos are within half an ulp, x 2.5; div_f32 within one ulp where IEEE division is
    within half, x 2; entering a sum of independently rounded items whose maximum over >= 256 rows is compared; observed at the
    three known configs: 0.8 .. 1.7), plus fp64_term."""
    return 4 * y.max + fp64_term(case)


_Y = {}


def yardstick(case, precision, tol=1e-4, itmax=10000, geometry=None):
    """Y[case, precision, tol, itmax, geometry]: (max, median) over rows of the emulation's relative distance from the oracle,
    the handed over items, the oracle's (log-L, flags).  Computed once a process."""
    key = (case.name, precision, tol, itmax, geometry if itmax > K_F32_STEPS else None)
    if key not in _Y:
        ref, rflags = oracle_of(case, tol, itmax)
        info = {}
        err = rel_err(emulate(case, precision, tol, itmax, info=info, geometry=geometry), ref)
        _Y[key] = SimpleNamespace(max=float(err.max()), median=float(np.median(err)), handed=info["handed"], ref=ref, rflags=rflags,
                                  items=case.theta.shape[0] * case.table.time.size * max(1, case.nplanets))
    return _Y[key]


# ---- the itmax marks of the single-item path (itmax = 5) --------------------------------------------------------------------

_PLACED = []


def placed_rows():
    """solver_cases.placed(200, 256) and, of its rows, those a float solver can be held to at itmax = 5: the first failing
    epoch of BOTH planets is the same by the fp64 counts and by the float counts, with numpy's float sin / cos and with them
    nudged one float ulp up and down (elsewhere a float and a double legitimately abort the array at different epochs).
    Returns (case, kept[rows], inside[rows]: a kept row with a mark strictly inside the array, unnudged agreement count)."""
    if not _PLACED:
        import solver_cases as sc
        case = sc.placed(*sc.PLACED_SHAPES[0])
        case.linpar, case.nplanets, case.n_epochs = {}, 2, case.table.time.size
        ne, names, rows = case.n_epochs, case.parnames, case.theta.shape[0]
        first = lambda fail: np.where(fail.any(axis=1), fail.argmax(axis=1), ne)
        keep, plain, inside = np.ones(rows, bool), np.ones(rows, bool), np.zeros(rows, bool)
        for p in (1, 2):
            period, ma0, ecc = (case.theta[:, names.index(f"planet{p}_{k}")] for k in ("period", "ma0", "ecc"))
            M = (TWO_PI / period)[:, None] * (case.table.time[None, :] - case.fixed[f"planet{p}_epoch"]) + ma0[:, None]
            f64 = first(sc.newton_counts(sincos_numpy, M, ecc[:, None], 1e-4, sc.PLACED_ITMAX) >= sc.PLACED_ITMAX)
            Mf, ecf = reduce_2pi_to_f32(M.ravel()), np.broadcast_to(ecc[:, None], M.shape).ravel().astype(f32)
            for k, sincos in enumerate((sincos_numpy, sincos_nudged(+1), sincos_nudged(-1))):
                steps = newton_f32(sincos, Mf, ecf, f32(1e-4), sc.PLACED_ITMAX)[4].reshape(M.shape)
                same = first(steps >= sc.PLACED_ITMAX) == f64
                keep &= same
                if k == 0:
                    plain &= same
            inside |= (f64 > 0) & (f64 < ne)
        _PLACED.append((case, keep, keep & inside, int(plain.sum())))
    return _PLACED[0]


def placed_kept_case():
    """The kept rows of placed_rows() as a case of their own (itmax = 5)."""
    import solver_cases as sc
    case, keep, _, _ = placed_rows()
    return SimpleNamespace(name="placed200_kept", table=case.table, parnames=case.parnames, fixed=case.fixed,
                           theta=np.ascontiguousarray(case.theta[keep]), linpar={}, nplanets=2, n_epochs=case.n_epochs,
                           runs=((1e-4, sc.PLACED_ITMAX),))
