"""The proposal walk and the resident live set at 46 to 129 parameters: the seeded model, the cases and the references shared by
tests/test_highdim_cases_host.py (the references alone meet every condition the GPU tests rely on), tests/test_gpu_walk_highdim.py
(the device walk move by move against tests/walk_replay.py) and tests/test_gpu_live_highdim.py (the live set's moments, order and
wide-row moves).

The model.  ndim free instrument offsets, no planet, one epoch an instrument (as _offsets_model of test_gpu_clustering.py), with
seeded data: vrad uniform in +-4, svrad uniform in 2 .. 5, priors Uniform(-10, 10).  Its log-L is an off-centre Gaussian of the
cube row u, centre (vrad + 10) / 20 in 0.3 .. 0.7 and width svrad / 20 in 0.1 .. 0.25 cube units; gaussian_evaluator() is the same
function in numpy, for the tests that have no GPU.  Coordinates 1 and ndim - 1 are wrapped (passed explicitly: an offset is not
circular by name; the walk wraps what it is told to).  With svrad = 0.1 (the sort tests' model) -0.5 log(2 pi s^2) = +1.38 a
term, so rows near the centre have log-L > 0 and the rest < 0: both branches of the device's sort key.

The dimension edges:
    walk          D <= 48 the whitening factor is staged in LDS (kWalkCholLds), from 49 it is read from global memory and every
                  LDS pointer behind chol_s moves; stepout ends at 64 (kStepoutMaxD), where the normals' top draw field 8191 sits
                  next to the first shrink draw 8192; walk_args shrinks the walker slots until PB D <= 1024 and the LDS fits.
    moments_cov   D D <= 2048 (D <= 45) the (j, l) sums stay in registers, from 46 they accumulate in global memory; a second
                  staging round beyond kMomBlocks kCovRows = 4096 rows.
    moments_sum   256 / D row groups a block: 2 at 128, 1 at 129; fewer than 128 rows leave blocks without any.

walk_lds() restates the LDS arithmetic of csrc/rvll_tile.h (carve), csrc/rvll_walk.hip (walk_lds_bytes) and the pointer chain of
csrc/rvll_walk_kernel.h for this model's layout, so that the slots a workgroup gets and the first refused dimension are computed
from the code's own formulas, not taken from a launch.
"""
from types import SimpleNamespace

import numpy as np

K_THREADS = 256               # rvll_kernels.h kThreads
K_TILE_WINDOW = 4096          # rvll_kernels.h kTileWindow (the handle's chunk_items)
K_WALK_CHOL_LDS = 48          # rvll_kernels.h kWalkCholLds
K_MAX_PB = 32                 # rvll_kernels.h kMaxPointsPerBlock
K_INST_DOUBLES = 4            # sizeof(rvll_inst) / 8: two slots of 16 bytes
K_SLOT_DOUBLES = 2            # sizeof(rvll_slot) / 8
DATA_SEED = 20240
TWO_PI = 2.0 * np.pi


def names(ndim):
    return [f"i{k:03d}" for k in range(ndim)]          # (zero-padded: theta is ordered as sorted(parnames))


def offsets_data(ndim, svrad=None, seed=DATA_SEED):
    """(vrad, svrad) of the ndim instruments' one epoch each; svrad: a constant instead of the seeded 2 .. 5."""
    rng = np.random.default_rng([seed, ndim])
    vrad = rng.uniform(-4.0, 4.0, ndim)
    s = rng.uniform(2.0, 5.0, ndim)
    return vrad, (s if svrad is None else np.full(ndim, float(svrad)))


def offsets_model(ndim, svrad=None, seed=DATA_SEED):
    """The GPU model (a context manager)."""
    from evidence_amd import GpuRVModel
    from evidence_amd import priors as P
    from evidence_amd.data import EpochTable
    vrad, s = offsets_data(ndim, svrad, seed)
    table = EpochTable.from_arrays(names(ndim), np.arange(1.0, ndim + 1.0), vrad, s, np.arange(ndim))
    pri = {f"{n}_offset": P.Uniform(-10, 10) for n in names(ndim)}
    return GpuRVModel({}, table, list(pri), priordict=pri)


def gaussian_evaluator(ndim, svrad=None, seed=DATA_SEED):
    """evaluate(cube) -> (theta, logl) of the same model in numpy: theta = -10 + 20 u, log-L the sum over the instruments of
    -0.5 ((vrad - theta) / svrad)^2 - 0.5 log(2 pi svrad^2)."""
    vrad, s = offsets_data(ndim, svrad, seed)
    norm = -0.5 * np.log(TWO_PI * s * s)

    def evaluate(c):
        theta = -10.0 + 20.0 * np.asarray(c, dtype=np.float64)
        z = (vrad - theta) / s
        return theta, np.sum(-0.5 * z * z + norm, axis=1)
    return evaluate


def wrapped(ndim):
    w = np.zeros(ndim, dtype=bool)
    w[1] = w[ndim - 1] = True
    return w


# ---- the walk cases: (name, ndim, proposal, rows drawn (half survive the quantile-0.5 cut), moves, start seed) ---------------
def _walk_cases():
    out = []
    for d in (48, 49, 64, 129):
        for proposal in ("chord", "stepout"):
            if proposal == "stepout" and d > 64:
                continue
            out.append(SimpleNamespace(name=f"D{d} {proposal}", ndim=d, proposal=proposal, k=600, nsteps=6, seed=100 + d))
    out.append(SimpleNamespace(name="D64 stepout redraw", ndim=64, proposal="stepout", k=64, nsteps=66, seed=264))
    for proposal in ("chord", "stepout"):
        out.append(SimpleNamespace(name=f"D49 queue {proposal}", ndim=49, proposal=proposal, k=1200, nsteps=9, seed=349))
    out.append(SimpleNamespace(name="D49 rounds", ndim=49, proposal="chord", k=16384, nsteps=3, seed=449))
    return out


WALK_CASES = _walk_cases()
WALK_CASE = {c.name: c for c in WALK_CASES}
RUN_MODE = SimpleNamespace(ndim=64, k=590, seed=564, sizes=(5, 60, 130, 100), steps=(8, 3, 5, 6))      # 295 rows survive
LIVE_STEP = SimpleNamespace(n=400, kdead=50, nsteps=4, base=1000, seed=99)                             # at D = 49 and 129


def run_mode_arguments(lstar, chol):
    """Four runs with their own lstar, factor and seed (test_run_mode_with_every_run_its_own_arguments' set)."""
    lst = np.array([lstar, lstar - 1.0, lstar - 0.25, lstar - 3.0])
    chols = np.stack([chol, 0.5 * chol, 2.0 * chol, 0.1 * chol])
    seeds = np.array([3, 2 ** 64 - 1, 5, 2 ** 63], dtype=np.uint64)
    return lst, chols, seeds


def live_step_case(ndim, logl_of):
    """The resident step of test_the_resident_live_step at ndim parameters: LIVE_STEP.n uniform rows, kdead die, the walkers
    start from `pick` among the survivors.  logl_of(cube) -> log-L [n] (live_init on the device, the evaluator on the host).
    Returns (cube, order, lstar, start rows)."""
    c = LIVE_STEP
    rng = np.random.default_rng([15, ndim])
    cube = rng.random((c.n, ndim))
    pick = rng.integers(0, c.n - c.kdead, c.kdead)
    logl = logl_of(cube)
    order = np.argsort(logl, kind="stable").astype(np.int32)
    return cube, order, float(logl[order[c.kdead - 1]]), order[c.kdead:][pick]


# ---- the whitening factor -------------------------------------------------------------------------------------------------------
FACTOR_CASES = [(7, 32), (45, 400), (46, 400), (64, 129), (64, 4097), (128, 300), (129, 300), (129, 4097)]      # (D, survivors)
FACTOR_KDEAD = 8
FACTOR_FLOOR = 1e-12          # the GPU bound is never looser than this, of max|L|
FACTOR_MARGIN = 64            # the device's other summation order: 128 block partials folded in quarters


def live_cube(ndim, survivors, kdead=FACTOR_KDEAD, seed=777):
    """survivors + kdead uniform live rows (as test_the_resident_live_step draws them); the kdead lowest in log-L die."""
    return np.random.default_rng([seed, ndim, survivors]).random((survivors + kdead, ndim))


def survivors_of(cube, logl, kdead=FACTOR_KDEAD):
    """(order, the rows that survive a step of kdead): numpy's stable order of logl."""
    order = np.argsort(logl, kind="stable").astype(np.int32)
    return order, cube[order[kdead:]]


def factor_reference(rows):
    """The whitening factor of `rows` [n, D] in numpy.longdouble: mean, d.T d / (n - 1), + 1e-14 on the diagonal, and the lower
    Cholesky - Banachiewicz factor by the loop of csrc/rvll_live_host.hip, whitening_factor.  Returns [D, D] longdouble."""
    ld = np.longdouble
    x = np.asarray(rows, dtype=np.float64).astype(ld)
    n, D = x.shape
    mean = x.sum(axis=0) / ld(n)
    d = x - mean
    cov = np.zeros((D, D), dtype=ld)
    for j in range(D):
        cov[j] = (d[:, j, None] * d).sum(axis=0)          # (longdouble throughout: no BLAS)
    cov /= ld(n - 1)
    cov[np.diag_indices(D)] += ld(1e-14)
    f = np.zeros((D, D), dtype=ld)
    for j in range(D):
        for l in range(j + 1):
            s = cov[j, l] - (f[j, :l] * f[l, :l]).sum()
            if j == l:
                assert s > 0
                f[j, j] = np.sqrt(s)
            else:
                f[j, l] = s / f[l, l]
    return f


def factor_distance(got, ref):
    """max |got - ref| / max |ref|, in longdouble."""
    return float(np.abs(np.asarray(got).astype(np.longdouble) - ref).max() / np.abs(ref).max())


def factor_bound(rows, ref=None):
    """The bound of the device's factor of `rows`: FACTOR_MARGIN times the distance of the float64 numpy factor
    (nested._whitening) from the longdouble reference, never looser than FACTOR_FLOOR (both of max|L|).  Returns (bound,
    the float64 distance, the reference)."""
    from evidence_amd.nested import _whitening
    ref = factor_reference(rows) if ref is None else ref
    host = factor_distance(_whitening(np.asarray(rows, dtype=np.float64)), ref)
    return min(FACTOR_MARGIN * host, FACTOR_FLOOR), host, ref


# ---- the order -----------------------------------------------------------------------------------------------------------------
SORT_NDIM, SORT_SVRAD = 7, 0.1


def sort_cube(n, ndup, seed):
    """n rows of the svrad = 0.1 model of which the last ndup repeat earlier rows exactly (ties in log-L, in rows far apart); a
    third of the rows within a width of the centre (log-L > 0), the rest uniform (log-L < 0)."""
    vrad, s = offsets_data(SORT_NDIM, SORT_SVRAD)
    rng = np.random.default_rng(seed)
    cube = rng.random((n, SORT_NDIM))
    near = rng.random(n) < 1.0 / 3.0
    cube[near] = np.clip((vrad + 10.0) / 20.0 + 0.4 * (s / 20.0) * rng.standard_normal((int(near.sum()), SORT_NDIM)), 0.0, np.nextafter(1.0, 0.0))
    src = rng.choice(n - ndup, ndup, replace=False)
    cube[n - ndup:] = cube[src]
    return cube


# ---- the walk kernel's LDS, restated -------------------------------------------------------------------------------------------
def carve_doubles(pb, ndim, ch):
    """rvll_tile.h carve() for Np = 0, Ni = ndim, nlin = 0: (offset of the contribution window, total), in doubles."""
    o = pb * ndim
    o = (o + 1) & ~1
    o += pb * ndim * 2 + pb * 6 + pb                                   # ins, dr, acc (pp and lin are empty)
    o += ndim * K_INST_DOUBLES + 5 * K_SLOT_DOUBLES                    # layout_doubles
    o = (o + 1) & ~1
    contrib = o
    o += ch
    o += (4 + 2 * pb + 1) // 2
    return contrib, o


def walk_window(pb, ndim):
    """walk_args' window(): the tile's contribution window, widened to the walk's 3 PB D doubles (Ne = ndim here)."""
    ch = min(K_TILE_WINDOW, max(K_THREADS, pb * ndim))
    return (max(ch, 3 * pb * ndim) + 1) & ~1


def walk_lds(pb, ndim, stepout):
    """(walk_lds_bytes(a, proposal), the last byte + 1 the kernel's pointer chain reaches, window doubles needed, window doubles)
    at PB = pb: rvll_walk.hip walk_lds_bytes against rvll_walk_kernel.h lines 72 - 118."""
    ch = walk_window(pb, ndim)
    contrib, total = carve_doubles(pb, ndim, ch)
    base = (8 * total + 15) & ~15
    chol = ndim * ndim if ndim <= K_WALK_CHOL_LDS else 0
    size = base + 8 * (2 * pb * ndim + 4 * pb + chol) + 4 * (16 * pb + 4 + ndim) + 16
    # the chain: wu, dir [PB][D]; tmin, tmax, slot_t, wl [PB]; chol_s; act [2][PB] and 14 int arrays [PB]; nact_s [4]; wrapped_s [D]
    end = 8 * ((total + 1) & ~1) + 8 * (2 * pb * ndim + 4 * pb + chol) + 4 * (16 * pb + 4 + ndim)
    if stepout:
        size += 16 + 8 * 2 * pb + 4 * 4 * pb
        end = (end + 15) // 16 * 16 + 8 * 2 * pb + 4 * 4 * pb           # cmin_s, cmax_s [PB]; phase_of, bas_g, bas_b, bas_n [PB]
    return size, end, 3 * pb * ndim, ch


def walk_slots(ndim, stepout, pb0=K_MAX_PB):
    """The walker slots a workgroup gets when the launch geometry asks for pb0 (set_points_per_block(32): the most): build_args'
    loop (the tile alone within 60 KiB), then walk_args' (the walk within 60 KiB and PB D <= 4 kThreads).  0: refused."""
    pb = pb0
    while pb > 1 and 8 * carve_doubles(pb, ndim, (min(K_TILE_WINDOW, max(K_THREADS, pb * ndim)) + 1) & ~1)[1] > 60 * 1024:
        pb -= 1
    while pb > 1 and (walk_lds(pb, ndim, stepout)[0] > 60 * 1024 or pb * ndim > 4 * K_THREADS):
        pb -= 1
    if walk_lds(pb, ndim, stepout)[0] > 64 * 1024 or pb * ndim > 4 * K_THREADS:
        return 0
    return pb


def first_refused_ndim():
    """The smallest ndim of this model family whose chord walk walk_args refuses: PB D > 4 kThreads at PB = 1 gives 1025; the LDS
    check (walk_lds_bytes > 64 KiB at PB = 1) comes first."""
    d = 2
    while walk_slots(d, False, 1):
        d += 1
    return d
