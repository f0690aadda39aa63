"""GPU: the hand-written trips of the fp64 shortcut loop (rvll_math.h: newton_trips_asm) against the compiled loop, bit for bit —
the solve by itself through debug-eval ops 40 .. 47 (every exit step, both exit parities in every wave, steps beyond pi/4 at
several evaluations, partial EXEC, uniform exits, one lane; and, replayed per wave, waves that run all their trips inside the
routine and leave it with lanes in both register sets beside waves that hand over), and the log-L kernels against the bits the parent commit's library
gave on the MI355X (tests/golden/newton_asm_parent.npz), in every launch shape, and against the checked loop (itmax = 8)."""
import ctypes as C
import functools
import hashlib
import subprocess
from pathlib import Path

import numpy as np
import pytest

import golden
import newton_cases as nc
from evidence_amd import GpuRVModel
from evidence_amd.synthetic import make_workload
from rotate_cases import HIPCC

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "hostshortcut.hip"
LIB = HERE / "native" / "libhostshortcut.so"
N_REC, K_SAFE, TOL = 8192, 8, 1e-4
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _p(a):
    return a.ctypes.data_as(dp)


@functools.lru_cache(maxsize=None)
def host_lib():
    """The host build of tests/native/hostshortcut.hip (same flags as tests/newton_cases.py's), or None without hipcc."""
    if not Path(HIPCC).exists():
        return None
    hdrs = list((HERE.parent / "evidence_amd" / "csrc").glob("*.h"))
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in [SRC] + hdrs):
        subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "--offload-arch=gfx950",
                        f"-I{HERE.parent / 'evidence_amd' / 'csrc'}", str(SRC), "-o", str(LIB)], check=True)
    return C.CDLL(str(LIB))


@functools.lru_cache(maxsize=None)
def records():
    """(M, e) of the 8192 seeded records."""
    rng = np.random.default_rng(7)
    e = rng.choice([0.0, 1e-6, 0.05, 0.2, 0.4, 0.6, 0.7, 0.8, 0.9, 0.95, 0.97, 0.99], N_REC)
    M = np.where(rng.random(N_REC) < 0.5, rng.uniform(-10, 10, N_REC), rng.uniform(-1e4, 1e4, N_REC))
    M.setflags(write=False)
    e.setflags(write=False)
    return M, e


@functools.lru_cache(maxsize=None)
def host_solves():
    """The host build on the records: (steps of the whole solve by newton_cases.solve, steps within the shortcut loop, the mask of
    evaluations with a step beyond pi/4, and s, c, dE as the shortcut loop leaves them — written out and by newton_shortcut)."""
    hs, hn = host_lib(), nc.host_lib()
    M, e = records()
    full_steps = nc.solve(hn, M, e, nc.FUSED, tol=TOL)[0]
    steps, beyond = np.empty(N_REC, dtype=np.int32), np.empty(N_REC, dtype=np.int32)
    s, c, dE = np.empty(N_REC), np.empty(N_REC), np.empty(N_REC)
    hs.hs_trace(_p(M), _p(e), C.c_long(N_REC), C.c_double(TOL), steps.ctypes.data_as(ip), beyond.ctypes.data_as(ip), _p(s), _p(c), _p(dE))
    s2, c2, dE2 = np.empty(N_REC), np.empty(N_REC), np.empty(N_REC)
    hs.hs_shortcut(_p(M), _p(e), C.c_long(N_REC), C.c_double(TOL), _p(s2), _p(c2), _p(dE2))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in ((s, s2), (c, c2), (dE, dE2)))
    return full_steps, steps, beyond, s, c, dE


def _device(m, M, e, first_op):
    """(s, c, dE, settled) of ops first_op .. first_op + 3 on the records (M, e)."""
    rec = np.stack([M, e], axis=1).reshape(-1)
    return [m.debug_eval(first_op + k, rec)[:M.size] for k in range(4)]


@pytest.fixture(scope="module")
def solves(gpu_required):
    if host_lib() is None or nc.host_lib() is None:
        pytest.skip("hipcc not available")
    return host_solves()


def test_records_cover_every_exit(solves):
    """What the bit comparison below rests on, from the host build's own counts: solves that stop after each of 1 .. 8 steps and
    solves still going then; a step beyond pi/4 (where the hand-written trips hand over) at two different evaluations or more;
    lanes of both exit parities in every wave of 64 records.  The figures are those of a plain numpy Newton iteration."""
    full_steps, steps, beyond, _, _, dE = solves
    settled = np.abs(dE) <= TOL
    assert np.array_equal(np.minimum(full_steps, K_SAFE)[settled], steps[settled]) and (full_steps[~settled] > K_SAFE).all()
    stops = [int((settled & (steps == k)).sum()) for k in range(1, K_SAFE + 1)]
    far = [int(((beyond >> k) & 1).sum()) for k in range(1, K_SAFE)]
    parity = steps.reshape(-1, 64) % 2
    mixed = int(((parity.min(axis=1) == 0) & (parity.max(axis=1) == 1)).sum())
    print(f"stops after 1 .. 8 steps {stops}, still going {int((~settled).sum())}, beyond pi/4 at evaluations 1 .. 7 {far}, "
          f"waves of mixed parity {mixed} of {parity.shape[0]}")
    assert stops == [1319, 1173, 2263, 1926, 982, 381, 68, 12] and int((~settled).sum()) == 68
    assert far == [1944, 633, 81, 74, 62, 56, 53]
    assert all(n > 0 for n in stops) and sum(n > 0 for n in far) >= 2 and mixed == parity.shape[0] == 128


def record_sets(steps, beyond, settled):
    """The launches of the bit comparison, as indices into the records.  The issue's: all; all but the last 37 (the last wave enters
    with partial EXEC); 64 copies of a record that stops after an odd count and of one that stops after an even count; one record.
    The exit of the hand-written trips is per WAVE — one active lane with a step beyond pi/4 hands the whole wave over — and every
    wave of "all" holds such a lane at evaluation 1 (test_waves_take_every_path), so these besides: the records without such a step,
    in whole waves and cut short by 37, whose waves run their trips in the routine to the end; and uniform waves of a record that
    goes beyond pi/4, of an odd and of an even step count."""
    near = np.flatnonzero(beyond == 0)
    near = near[:near.size // 64 * 64]
    pick = lambda sel: int(np.flatnonzero(sel)[0])
    odd, even = pick(settled & (steps == 3) & (beyond == 0)), pick(settled & (steps == 4) & (beyond == 0))
    far_odd, far_even = pick(settled & (beyond != 0) & (steps == 5)), pick(settled & (beyond != 0) & (steps == 6))
    return {"all": np.arange(N_REC), "partial": np.arange(N_REC - 37), "odd": np.full(64, odd), "even": np.full(64, even),
            "one": np.array([odd]), "near": near, "near partial": near[:-37], "beyond odd": np.full(64, far_odd),
            "beyond even": np.full(64, far_even), "one beyond": np.array([far_odd])}


def wave_paths(steps, beyond):
    """What newton_trips_asm does with each wave of 64 lanes, replayed from the host build's per-lane step counts and beyond-pi/4
    masks: (evaluation at which it hands over to the compiled loop or 0, half-trips it ran, lanes on entry, lanes that leave with
    their state in set B, lanes that leave with it in set A, whether EXEC narrowed between two half-trips).  A lane is active at
    evaluation k while its solve takes more than k steps; evaluation k is half A for odd k and half B for even k; a lane that took
    its last step in half A (an even step count) leaves with its state in set B."""
    out = []
    for w0 in range(0, steps.size, 64):
        st, by = steps[w0:w0 + 64], beyond[w0:w0 + 64]
        bail, ran, narrowed, last = 0, 0, False, None
        for k in range(1, K_SAFE):
            act = st > k
            if not act.any():
                break
            if (act & (((by >> k) & 1) == 1)).any():
                bail = k
                break
            narrowed |= last is not None and int(act.sum()) < last
            last = int(act.sum())
            ran += 1
        done = np.minimum(st, (bail if bail else K_SAFE))           # steps taken when the lane leaves the routine
        in_b = int(((done % 2 == 0) & (done > 1)).sum())
        out.append((bail, ran, st.size, in_b, st.size - in_b, narrowed))
    return out


def test_waves_take_every_path(solves):
    """The coverage of the hand-written trips themselves, per wave (wave_paths), over the launches of the bit comparison: waves that
    finish inside the routine with lanes in both register sets, after a half A and after a half B, with EXEC narrowing between
    half-trips, entered with partial EXEC; waves that hand over with nothing yet in set B; uniform waves.  On these records —
    and on 8 million more drawn at e = 0.9 .. 0.99 with |M| up to 1e4 and up to 2^48, checked once by hand — a solve from E = M
    whose first step is within pi/4 never takes a later one beyond it (Newton's steps on E - e sin E shrink once one is that
    small), so a hand-over always falls at evaluation 1, in the first half A, before any lane's state is in set B: asserted here,
    so that a record set which does reach a later hand-over is noticed."""
    _, steps, beyond, _, _, dE = solves
    settled = np.abs(dE) <= TOL
    assert np.array_equal(beyond != 0, ((beyond >> 1) & 1) == 1)
    paths = {name: wave_paths(steps[idx], beyond[idx]) for name, idx in record_sets(steps, beyond, settled).items()}
    for name, p in paths.items():
        print(f"{name}: {len(p)} waves, {sum(b > 0 for b, *_ in p)} hand over, half-trips run {sorted({r for _, r, *_ in p})}, "
              f"{sum(b == 0 and nb > 0 and na > 0 for b, _, _, nb, na, _ in p)} finish inside with lanes in both sets")
    assert all(b == 1 and r == 0 for b, r, *_ in paths["all"]) and len(paths["all"]) == 128
    for name in ("near", "near partial"):
        p = paths[name]
        assert len(p) == 97 and all(b == 0 for b, *_ in p)
        assert all(nb > 0 and na > 0 and narrowed for _, _, _, nb, na, narrowed in p)        # both sets, EXEC narrowed, in every wave
        assert {r % 2 for _, r, *_ in p} == {0, 1} and max(r for _, r, *_ in p) >= 5          # left after a half A and after a half B
    assert paths["near partial"][-1][2] == 27 and paths["partial"][-1][2] == 27
    assert paths["odd"] == [(0, 2, 64, 0, 64, False)] and paths["even"] == [(0, 3, 64, 64, 0, False)]
    assert paths["beyond odd"][0][:2] == (1, 0) and paths["beyond even"][0][:2] == (1, 0) and paths["one beyond"][0][:3] == (1, 0, 1)


def test_solve_hand_written_equals_compiled_bit_for_bit(solves):
    """Ops 40 .. 43 (first trip compiled, the later ones hand-written, the compiled loop after a step beyond pi/4) against ops
    44 .. 47 (the compiled loop throughout) in the same launch geometry, on every launch of record_sets.  Settled records against
    the host build as well."""
    _, steps, beyond, hs_, hc_, hdE = solves
    M, e = records()
    settled = np.abs(hdE) <= TOL
    sets = record_sets(steps, beyond, settled)
    w = make_workload(1)
    with GpuRVModel(w.fixedpardict, w.table, w.parnames) as m:
        for name, idx in sets.items():
            asm = _device(m, M[idx], e[idx], 40)
            cmp = _device(m, M[idx], e[idx], 44)
            for what, a, b in zip(("s", "c", "dE", "settled"), asm, cmp):
                assert np.array_equal(_bits(a), _bits(b)), (name, what, int((_bits(a) != _bits(b)).sum()))
            ok = settled[idx]
            assert np.array_equal(asm[3] == 1.0, ok), name
            for what, a, h in zip(("s", "c", "dE"), asm, (hs_[idx], hc_[idx], hdE[idx])):
                assert np.array_equal(_bits(a[ok]), _bits(h[ok])), (name, what, "host")


@pytest.fixture(scope="module", params=[1, 2, 3], ids=["np1", "np2", "np3"])
def case(request):
    return request.param, nc.gpu_case(request.param)


def test_kernels_give_the_parent_commits_bits(gpu_required, case):
    """log-L and flags of newton_cases.gpu_case(1 | 2 | 3) as raw bits against the record made with the PARENT commit's library on
    the MI355X (tests/golden/newton_asm_parent.npz; never regenerated from the tree under test): the default launch, both kernel
    forms at 1, 2 and 7 points a block, permuted, and one row a launch."""
    npl, (table, free, fixed, theta) = case
    z = np.load(golden.GOLDEN / "newton_asm_parent.npz")
    assert hashlib.sha256(np.ascontiguousarray(theta).tobytes()).digest() == z[f"theta_sha256_np{npl}"].tobytes()
    want, wflags = z[f"logl_bits_np{npl}"], z[f"flags_np{npl}"]
    n = theta.shape[0]
    perm = np.random.default_rng(5).permutation(n)
    with GpuRVModel(fixed, table, free) as m:
        got = m.log_likelihood_batch(theta, return_flags=True)
        assert np.array_equal(_bits(got[0]), want) and np.array_equal(got[1], wflags), "default"
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            for pb in (1, 2, 7):
                m.set_points_per_block(pb)
                got = m.log_likelihood_batch(theta, return_flags=True)
                assert np.array_equal(_bits(got[0]), want) and np.array_equal(got[1], wflags), (form, pb)
                got = m.log_likelihood_batch(theta[perm], return_flags=True)
                assert np.array_equal(_bits(got[0]), want[perm]) and np.array_equal(got[1], wflags[perm]), (form, pb, "perm")
        m.set_points_per_block(0)
        m.set_kernel_form("auto")
        singles = [m.log_likelihood_batch(theta[i:i + 1], return_flags=True) for i in range(n)]
    assert np.array_equal(_bits(np.concatenate([s[0] for s in singles])), want)
    assert np.array_equal(np.concatenate([s[1] for s in singles]), wflags)


def test_checked_loop_gives_the_same_bits(gpu_required, case):
    """itmax = 8 turns the shortcut off and runs the compiled checked loop: on the rows whose solves all settle within seven steps
    (the oracle's own counts) it gives the default launch's bits and flags, in both kernel forms."""
    from evidence_amd.layout import compile_layout
    from oracle.oracle import OracleModel
    _, (table, free, fixed, theta) = case
    om = OracleModel(compile_layout(free, fixed, table.insts, []), table)
    settled = np.array([om.iteration_counts(x).max() <= 7 for x in theta])
    assert settled.sum() >= theta.shape[0] // 3
    with GpuRVModel(fixed, table, free) as m:
        base, flags = m.log_likelihood_batch(theta, return_flags=True)
    with GpuRVModel(fixed, table, free, itmax=8) as m:
        for form in ("tile", "cu"):
            m.set_kernel_form(form)
            got = m.log_likelihood_batch(theta, return_flags=True)
            assert np.array_equal(_bits(got[0][settled]), _bits(base[settled])), form
            assert np.array_equal(got[1][settled], flags[settled]), form
