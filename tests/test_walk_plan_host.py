"""CPU: the integer decisions of the device walk's host driver (evidence_amd/csrc/rvll_walk_plan.h: the RVLL_WALK_* / RVLL_ROUNDS_*
switches, the geometry of a walk in rounds and the layout of its arena, the single-kernel walk's tile, the two-part rule, the order
and the deal of the second part's rows, the wide rows form), compiled alone for the host (tests/native/walkplan.cpp) and held against
a second statement of the rules in Python and numpy.  What the library asks its kernels' launch interface (LDS sizes, occupancy) is
a stand-in on both sides.  Needs a host C++ compiler."""
import ctypes as C
import itertools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "walkplan.cpp"
INC = HERE.parent / "evidence_amd" / "csrc"
THREADS, WAVE, MAX_POINTS, CU_THREADS, CU_MAX_POINTS, RING, MAX_GROUPS = 256, 64, 32, 1024, 128, 16, 4
LDS, LDS_MAX, CU_LDS = 60 * 1024, 64 * 1024, 156 * 1024
CHUNK = 4096                                             # the tile's contribution window (rvll::kTileWindow)
SWITCHES = ("RVLL_WALK_ROUNDS", "RVLL_WALK_QUEUE", "RVLL_WALK_PARTS", "RVLL_WALK_ROWS", "RVLL_WALK_FAT", "RVLL_WALK_SPEC", "RVLL_WALK_CR",
            "RVLL_WALK_FIRST", "RVLL_WALK_GEOM_DUMP", "RVLL_WALK_COST_DUMP", "RVLL_WALK_TILE_DUMP", "RVLL_ROUNDS_GROUPS", "RVLL_ROUNDS_FREE",
            "RVLL_ROUNDS_FORM", "RVLL_ROUNDS_PER", "RVLL_ROUNDS_W", "RVLL_ROUNDS_PB", "RVLL_ROUNDS_STAMPS", "RVLL_ROUNDS_DEPTH",
            "RVLL_ROUNDS_LISTED_DUMP", "RVLL_ROUNDS_CHAIN", "RVLL_ROUNDS_PRIO")
# the variants of test_gpu_walk.py::test_rounds_form_is_the_single_kernel_walk, and rows a group that leave an unequal last group
VARIANTS = [{}, {"RVLL_ROUNDS_GROUPS": "1"}, {"RVLL_ROUNDS_GROUPS": "2", "RVLL_ROUNDS_FORM": "cu"}, {"RVLL_ROUNDS_GROUPS": "4", "RVLL_WALK_SPEC": "1"},
            {"RVLL_ROUNDS_GROUPS": "2"}, {"RVLL_ROUNDS_CHAIN": "1"}, {"RVLL_ROUNDS_PRIO": "1", "RVLL_ROUNDS_W": "16"},
            {"RVLL_WALK_SPEC": "16", "RVLL_ROUNDS_FREE": "100000"}, {"RVLL_ROUNDS_FREE": "1", "RVLL_ROUNDS_DEPTH": "1"},
            {"RVLL_ROUNDS_DEPTH": "9", "RVLL_ROUNDS_PB": "3"}, {"RVLL_ROUNDS_PER": "1700"}]


def _compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return [shutil.which(name)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if Path(hipcc).exists() else None


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("walkplan") / "libwalkplan.so"
    subprocess.run(cxx + ["-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror", f"-I{INC}", str(SRC), "-o", str(out)], check=True)
    so = C.CDLL(str(out))
    so.wp_order.restype = so.wp_deal.restype = C.c_int64
    return so


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ids(env):
    return "-".join(f"{k[5:]}={v}" for k, v in env.items()) or "unset"


# ---- the stand-ins (tests/native/walkplan.cpp states the three LDS sizes alike) -----------------------------------------------------
def tile_lds(D, PB, CH):
    return 8 * (CH + PB * (2 * D + 24)) + 2048


def walk_lds(D, PB, CH):
    return 8 * (CH + PB * (5 * D + 40)) + 4096


def rows_lds(D, PB, CH, rows):
    return walk_lds(D, PB, CH) + 8 * rows * (2 * D + 4)


def step_walkers(D, spec):
    """walkers a step workgroup holds within 60 KiB (0: not one within 64 KiB)"""
    lds = lambda W: 8 * W * (4 * D + 2 * spec + 6) + 4 * (2 * W * spec + 8 * W + 4 + D)         # noqa: E731
    W = WAVE
    while W > 1 and lds(W) > LDS:
        W -= 1
    return W if lds(W) <= LDS_MAX else 0


def _window(pb, Ne):
    return (min(CHUNK, max(THREADS, pb * Ne)) + 1) & ~1


def base_tile(D, Ne, B):
    """a cost model's tile for a batch of B points, shrunk to the 60 KiB budget as build_args shrinks it"""
    pb = 8 if B >= 4096 else 4 if B >= 512 else 2
    while pb > 1 and tile_lds(D, pb, _window(pb, Ne)) > LDS:
        pb -= 1
    return pb, _window(pb, Ne)


def occupancy(lds):
    return min(8, (160 * 1024) // lds)


# ---- the rules, stated again ----------------------------------------------------------------------------------------------------
def _int(env, name, default=None):
    return int(env[name]) if name in env else default


def want_start(K, n_cu, Ne, spec, env):
    spec = max(1, min(_int(env, "RVLL_WALK_SPEC", spec), MAX_POINTS))
    G = max(1, min(_int(env, "RVLL_ROUNDS_GROUPS", 3), MAX_GROUPS, K))
    c_free = max(1, _int(env, "RVLL_ROUNDS_FREE")) if "RVLL_ROUNDS_FREE" in env else max(256, n_cu * 4608 // max(1, Ne))
    per = max(1, min(K, _int(env, "RVLL_ROUNDS_PER"))) if "RVLL_ROUNDS_PER" in env else -(-K // G)
    return G, spec, per, c_free, max(per, c_free)


def want_plan(K, D, Ne, n_cu, nsteps, max_rounds, spec, PB0, CH0, occ, W0, env):
    """None: refused; else the plan's fields in wp_plan's order"""
    _, spec, per, c_free, _ = want_start(K, n_cu, Ne, spec, env)
    cu = env.get("RVLL_ROUNDS_FORM") == "cu"
    depth = max(1, _int(env, "RVLL_ROUNDS_DEPTH", 4))
    if W0 < 1:
        return None
    W = max(1, min(W0, _int(env, "RVLL_ROUNDS_W", W0)))
    per = -(-per // W) * W
    G = -(-K // per)
    C, nblk = max(per, c_free), per // W
    c_free = min(c_free, C)
    if C >= 1 << 30 or per * spec >= 1 << 31 or G > MAX_GROUPS:
        return None
    PB, CH = PB0, CH0
    if cu:
        PB = min(CU_MAX_POINTS, -(-C // n_cu))
        fits = lambda q: tile_lds(D, q, (q * Ne + 1) & ~1) <= CU_LDS                              # noqa: E731
        while PB > 1 and not fits(PB):
            PB -= 1
        if not fits(PB):
            return None
        CH = (PB * Ne + 1) & ~1
    else:
        room = max(1, occ) * n_cu - (nblk if G > 1 else 0)
        want = -(-C // room) if room > 0 else PB
        if PB < want <= MAX_POINTS and tile_lds(D, want, _window(want, Ne)) <= LDS:
            PB, CH = want, _window(want, Ne)
        if "RVLL_ROUNDS_PB" in env:
            pb = max(1, min(int(env["RVLL_ROUNDS_PB"]), MAX_POINTS))
            if tile_lds(D, pb, _window(pb, Ne)) <= LDS:
                PB, CH = pb, _window(pb, Ne)
    return (1, int(cu), G, W, spec, PB, CH, -(-C // PB), depth, per, C, c_free, nblk, nsteps * max_rounds + 2 + depth, tile_lds(D, PB, CH))


def _plan(lib, K, D, Ne, n_cu, nsteps, max_rounds, spec, PB0, CH0, occ, W0):
    plan, arena = np.zeros(15, np.int64), np.zeros(22, np.int64)
    lib.wp_plan(_ptr(np.array([K, D, Ne, n_cu, nsteps, max_rounds, spec, CHUNK, PB0, CH0, occ, W0], np.int64)), _ptr(plan), _ptr(arena))
    return tuple(int(v) for v in plan), [int(v) for v in arena]


def _check_arena(arena, per, C, nblk, D, spec):
    n_dbl, n_ll, n_int, g_bytes = arena[:4]
    offsets, zeroed = arena[4:21], arena[21]
    assert n_dbl == 2 * per * D + 2 * per + 2 * C * D + 2 * per * spec + C          # the driver's formulas before the arena had a layout
    assert n_ll == 2 * nblk + RING and n_int == 4 * per + 2 * per * spec + 2 * C
    up16 = lambda b: (b + 15) & ~15                                                                  # noqa: E731
    assert g_bytes == up16(8 * n_dbl) + up16(8 * n_ll) + up16(4 * n_int)
    # dir, dirnext, tmin, tmax, theta_c[0], theta_c[1], wt, wres_logl, res_logl | calls_part, slots_part, ring | ws, wres_flags, wdef, res_flags, owner
    sizes = [8 * n for n in (per * D, per * D, per, per, C * D, C * D, per * spec, per * spec, C, nblk, nblk, RING)] + \
            [4 * n for n in (4 * per, per * spec, per * spec, C, C)]
    ends = [o + s for o, s in zip(offsets, sizes)]
    assert offsets[0] == 0 and all(e <= o for e, o in zip(ends, offsets[1:])) and ends[-1] <= g_bytes      # in order, apart, inside the slice
    assert all(o % 8 == 0 for o in offsets[:12]) and all(o % 4 == 0 for o in offsets[12:])
    assert offsets[0] % 16 == 0 and offsets[9] % 16 == 0 and offsets[12] % 16 == 0 and g_bytes % 16 == 0    # the three sections, the next slice
    assert offsets[9] == up16(8 * n_dbl) and offsets[12] == offsets[9] + up16(8 * n_ll)
    assert all(e == o for e, o in zip(ends[:8], offsets[1:9])) and all(e == o for e, o in zip(ends[9:11], offsets[10:12])) and \
        all(e == o for e, o in zip(ends[12:16], offsets[13:17]))                                            # no holes inside a section
    assert zeroed == offsets[12] - offsets[9]                                                               # the 64-bit section, whole


@pytest.mark.parametrize("env", VARIANTS, ids=_ids)
def test_rounds_plan_and_arena_over_the_grid(lib, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    refused = 0
    for K, D, Ne, n_cu, spec, max_rounds in itertools.product((1, 40, 131, 600, 5000, 6143, 6144, 16384, 24576, 24577), (1, 5, 19, 74, 129),
                                                              (1, 200, 5000), (1, 8, 256), (1, 8, 16), (1, 3, 4096)):
        nsteps = 9
        start = want_start(K, n_cu, Ne, spec, env)
        out = np.zeros(5, np.int64)
        lib.wp_start(C.c_int64(K), n_cu, Ne, spec, _ptr(out))
        assert tuple(out) == start, (K, D, Ne, n_cu, spec)
        PB0, CH0 = base_tile(D, Ne, start[4])
        occ, W0 = occupancy(tile_lds(D, PB0, CH0)), step_walkers(D, start[1])
        got, arena = _plan(lib, K, D, Ne, n_cu, nsteps, max_rounds, spec, PB0, CH0, occ, W0)
        want = want_plan(K, D, Ne, n_cu, nsteps, max_rounds, spec, PB0, CH0, occ, W0, env)
        case = (K, D, Ne, n_cu, spec, max_rounds, env)
        if want is None:
            assert got[0] == 0, case
            refused += 1
            continue
        assert got == want, case
        _, cu, G, W, sp, PB, CH, tiles, depth, per, Cs, c_free, nblk, r_max, lds = got
        assert per % W == 0 and (G - 1) * per < K <= G * per and 1 <= G <= MAX_GROUPS and 1 <= W <= WAVE, case
        assert 1 <= c_free <= Cs and Cs >= per and tiles * PB >= Cs > (tiles - 1) * PB and nblk * W == per, case
        assert lds <= (CU_LDS if cu else LDS) and 1 <= PB <= (CU_MAX_POINTS if cu else MAX_POINTS), case
        assert CH >= PB * Ne if cu else CH <= CHUNK + 1, case                    # CU-wide: every contribution of the tile resident
        _check_arena(arena, per, Cs, nblk, D, sp)
    if "RVLL_ROUNDS_PER" in env:
        assert refused > 0          # 1700 rows a group at 16384 rows and more: more groups than the handle has streams for
    elif "RVLL_ROUNDS_FORM" not in env:
        assert refused == 0


def test_rounds_plan_refusals(lib, monkeypatch):
    """What today's driver answers with RVLL_E_UNSUPPORTED: no walker fits a step workgroup, 2^30 candidate slots, 2^31 walker
    candidates, a CU-wide tile that does not hold one point — and more groups than the handle has streams and progress words for,
    which RVLL_ROUNDS_PER could ask for."""
    def refused(K, D=5, Ne=200, n_cu=256, spec=8, W0=64):
        PB0, CH0 = base_tile(D, Ne, K)
        got, _ = _plan(lib, K, D, Ne, n_cu, 9, 5, spec, PB0, CH0, 4, W0)
        want = want_plan(K, D, Ne, n_cu, 9, 5, spec, PB0, CH0, 4, W0, dict(__import__("os").environ))
        assert (want is None) == (got[0] == 0)
        return got[0] == 0
    assert not refused(5000) and refused(5000, W0=0)
    monkeypatch.setenv("RVLL_ROUNDS_FREE", str((1 << 30) - 1))
    assert not refused(5000)
    monkeypatch.setenv("RVLL_ROUNDS_FREE", str(1 << 30))
    assert refused(5000)
    monkeypatch.delenv("RVLL_ROUNDS_FREE")
    monkeypatch.setenv("RVLL_ROUNDS_GROUPS", "1")
    assert refused(1 << 27, spec=16) and not refused((1 << 27) - 64, spec=16) and not refused(1 << 27, spec=15)
    monkeypatch.delenv("RVLL_ROUNDS_GROUPS")
    monkeypatch.setenv("RVLL_ROUNDS_FORM", "cu")
    assert not refused(5000, Ne=5000) and refused(5000, Ne=20000)               # 20000 contributions of one point: 160 KB
    monkeypatch.delenv("RVLL_ROUNDS_FORM")
    monkeypatch.setenv("RVLL_ROUNDS_PER", "1280")
    assert not refused(5120) and refused(5121)


def test_switches_unset_set_and_out_of_range(lib, monkeypatch):
    def read():
        out = np.zeros(24, np.int64)
        lib.wp_switches(_ptr(out))
        return out.tolist()
    #        rounds sk queue one rows fat spec cr first_set first geom cost tile groups free cu per_set per w pb stamps depth listed chain|prio<<1
    assert read() == [-1, 0, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0]
    values = ("1", "5", "1", "2", "", "7", "1", "3", "", "1", "0", "2", "900", "cu", "1700", "16", "3", "12", "9", "", "1", "1")
    for name, value in zip(SWITCHES, values):
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("RVLL_WALK_ROWSS", "3")               # another name that begins like a switch's
    monkeypatch.setenv("RVLL_ROUNDS_MODE", "streams")        # a switch of earlier rounds that is no longer read
    assert read() == [1, 1, 5, 1, 2, 1, 7, 1, 1, 3, 1, 1, 1, 2, 900, 1, 1, 1700, 16, 3, 12, 9, 1, 3]
    low = {"RVLL_WALK_ROUNDS": "0", "RVLL_WALK_QUEUE": "-4", "RVLL_WALK_PARTS": "2", "RVLL_WALK_ROWS": "0", "RVLL_WALK_SPEC": "0",
           "RVLL_WALK_FIRST": "-3", "RVLL_ROUNDS_GROUPS": "-1", "RVLL_ROUNDS_FREE": "0", "RVLL_ROUNDS_FORM": "tile", "RVLL_ROUNDS_PER": "-5",
           "RVLL_ROUNDS_W": "0", "RVLL_ROUNDS_PB": "0", "RVLL_ROUNDS_STAMPS": "-1", "RVLL_ROUNDS_DEPTH": "0", "RVLL_ROUNDS_CHAIN": "0",
           "RVLL_ROUNDS_PRIO": "0", "RVLL_WALK_CR": "0"}
    for name, value in low.items():
        monkeypatch.setenv(name, value)
    assert read() == [0, 1, 0, 0, 0, 1, 1, 0, 1, -3, 1, 1, 1, -1, 1, 0, 1, -5, 1, 1, 0, 1, 1, 0]
    for name, value in (("RVLL_WALK_ROWS", "3"), ("RVLL_WALK_SPEC", "99"), ("RVLL_ROUNDS_PB", "99"), ("RVLL_ROUNDS_STAMPS", "99999"),
                        ("RVLL_WALK_QUEUE", "1000"), ("RVLL_ROUNDS_W", "1000")):
        monkeypatch.setenv(name, value)
    got = read()
    assert (got[4], got[6], got[19], got[20], got[2], got[18]) == (3, 32, 32, 4096, 1000, 1000)
    monkeypatch.setenv("RVLL_WALK_ROWS", "7")                # any other positive value: the 256-thread rows form
    assert read()[4] == 1
    assert lib.wp_max_cus(256) == 256 and lib.wp_max_cus(2000) == 1000       # the queue's clamp to the chip, where the chip is known
    # what clamps where K / nsteps are known: groups to 1 .. min(4, K), rows a group to 1 .. K, the first part to 1 .. nsteps - 1
    out = np.zeros(5, np.int64)
    lib.wp_start(C.c_int64(5000), 256, 200, 8, _ptr(out))
    assert tuple(out[:3]) == (1, 32, 1)
    monkeypatch.setenv("RVLL_ROUNDS_PER", "999999")
    lib.wp_start(C.c_int64(5000), 256, 200, 8, _ptr(out))
    assert out[2] == 5000


def test_rounds_are_wanted_by_size_unless_a_switch_says(lib, monkeypatch):
    wanted = lambda K: bool(lib.wp_rounds_wanted(C.c_int64(K)))                                         # noqa: E731
    assert [wanted(K) for K in (1, 6143, 6144, 16384, 24576, 24577, 40000)] == [False, False, True, True, True, False, False]
    for name, value in (("RVLL_WALK_QUEUE", "1"), ("RVLL_WALK_PARTS", "0"), ("RVLL_WALK_ROWS", "0"), ("RVLL_WALK_FAT", "")):
        monkeypatch.setenv(name, value)                      # set, whatever to: a single-kernel form is being tested or measured
        assert not wanted(16384)
        monkeypatch.setenv("RVLL_WALK_ROUNDS", "1")          # ... unless the rounds are asked for beside it
        assert wanted(16384) and wanted(40)
        monkeypatch.setenv("RVLL_WALK_ROUNDS", "0")
        assert not wanted(16384)
        monkeypatch.delenv("RVLL_WALK_ROUNDS")
        monkeypatch.delenv(name)
    monkeypatch.setenv("RVLL_WALK_ROUNDS", "0")
    assert not wanted(16384)
    monkeypatch.setenv("RVLL_WALK_ROUNDS", "2")
    assert wanted(1) and wanted(40000)


def test_single_kernel_tile(lib):
    def want(PB0, D, Ne, override, n):
        def window(pb):
            return (max(min(CHUNK, max(THREADS, pb * Ne)), 3 * pb * D) + 1) & ~1
        pb = PB0
        if override <= 0 and n >= 4096:
            pb = 10
            while pb > 1 and 4 * walk_lds(D, pb, window(pb)) > CU_LDS:
                pb -= 1
        big = lambda q, lds: walk_lds(D, q, window(q)) > lds or q * D > 4 * THREADS                      # noqa: E731
        while pb > 1 and big(pb, LDS):
            pb -= 1
        return (int(not big(pb, LDS_MAX)), pb, window(pb))
    seen = set()
    for PB0, D, Ne, override, n in itertools.product((1, 8, 32), (1, 5, 19, 74, 129, 300, 1025), (1, 200, 5000), (0, 6), (100, 4095, 4096, 40000)):
        out = np.zeros(3, np.int64)
        lib.wp_walk_tile(PB0, D, Ne, CHUNK, override, C.c_int64(n), _ptr(out))
        assert tuple(out) == want(PB0, D, Ne, override, n), (PB0, D, Ne, override, n)
        seen.add((int(out[0]), int(out[1])))
        if out[0]:
            assert walk_lds(D, out[1], out[2]) <= LDS_MAX and out[1] * D <= 4 * THREADS and out[2] >= 3 * out[1] * D
    assert (1, 10) in seen and (1, 1) in seen and (0, 1) in seen       # the 10-slot preference, shrunk to one walker, refused (1025 parameters)


def test_two_parts_first_part_and_rows_form(lib, monkeypatch):
    def parts(K, resident, PB, D, CH, nsteps):
        out = np.zeros(4, np.int64)
        lib.wp_parts(C.c_int64(K), C.c_int64(resident), PB, D, CH, nsteps, _ptr(out))
        return tuple(int(v) for v in out)
    assert parts(10241, 1024, 10, 19, 4096, 8) == (1, 0, 1, 2)             # more rows than walker slots, 8 moves: two parts
    assert parts(10240, 1024, 10, 19, 4096, 8)[0] == 0 and parts(10241, 1024, 10, 19, 4096, 7)[0] == 0 and parts(10241, 0, 10, 19, 4096, 8)[0] == 0
    assert parts(40000, 1024, 10, 19, 4096, 100)[2:] == (12, 25) and parts(40000, 1024, 10, 19, 4096, 3)[2:] == (1, 1)
    monkeypatch.setenv("RVLL_WALK_PARTS", "1")
    assert parts(10241, 1024, 10, 19, 4096, 8)[0] == 0
    monkeypatch.setenv("RVLL_WALK_PARTS", "2")
    assert parts(10241, 1024, 10, 19, 4096, 8)[0] == 1
    for first, want in (("5", 5), ("0", 1), ("99", 19), ("-2", 1)):
        monkeypatch.setenv("RVLL_WALK_FIRST", first)
        assert parts(40000, 1024, 10, 19, 4096, 20)[2:] == (want, want)
    assert parts(40000, 1024, 10, 19, 4096, 1)[2:] == (1, 1)               # (nsteps - 1 = 0: still one move)
    for rows in ("1", "2", "3"):
        monkeypatch.setenv("RVLL_WALK_ROWS", rows)
        assert parts(40000, 1024, 10, 19, 570, 20)[1] == 1 and parts(40000, 1024, 10, 19, 569, 20)[1] == 0    # 3 PB D candidates parked in the window
    monkeypatch.setenv("RVLL_WALK_ROWS", "0")
    assert parts(40000, 1024, 10, 19, 4096, 20)[1] == 0


def _order(lib, cost, done, first, max_rounds):
    cost, done = np.asarray(cost, np.int32), np.asarray(done, np.int32)
    order = np.full(len(cost), -1, np.int32)
    K2 = lib.wp_order(_ptr(cost), _ptr(done), C.c_int64(len(cost)), first, max_rounds, _ptr(order))
    return order, int(K2)


def test_order_by_cost(lib):
    rng = np.random.default_rng(5)
    for K, first, max_rounds in ((1, 2, 5), (37, 2, 5), (5000, 4, 200), (20000, 300, 4096)):
        cmax = min(first * max_rounds, 1 << 16)
        cost = rng.integers(-3, cmax + 50, K).astype(np.int32)             # below 0 and above cmax: held to 0 .. cmax
        done = np.where(rng.random(K) < 0.1, rng.integers(0, first, K), first + rng.integers(0, 2, K)).astype(np.int32)
        order, K2 = _order(lib, cost, done, first, max_rounds)
        assert np.array_equal(np.sort(order), np.arange(K))                # a permutation of the rows
        deferred = done < first
        assert K2 == K - deferred.sum() and deferred[order[K2:]].all() and not deferred[order[:K2]].any()
        key = np.clip(cost, 0, cmax)
        assert (np.diff(key[order[:K2]]) <= 0).all()                        # most expensive first
        # ... and stable: the whole order is numpy's stable sort by (deferred, -cost held to its range)
        assert np.array_equal(order, np.argsort(np.where(deferred, cmax + 1, cmax - key), kind="stable"))
    order, K2 = _order(lib, [70000, 65536, 65537, -1, 0, 3], [300] * 6, 300, 4096)      # above 65536 and below 0: one key each with the ends
    assert order.tolist() == [0, 1, 2, 5, 3, 4] and K2 == 6
    order, K2 = _order(lib, [5, 6, 7], [0, 0, 0], 1, 3)                                # every row deferred
    assert order.tolist() == [0, 1, 2] and K2 == 0


def test_deal_first_rows(lib):
    for K2, PB, resident in ((100, 8, 4), (33, 8, 4), (31, 8, 4), (5, 8, 4), (8, 8, 1), (1, 10, 1024), (20000, 10, 1024), (10239, 10, 1024)):
        for extra in (0, 7):                                                           # (deferred rows behind the K2 that go on)
            order = np.arange(1000, 1000 + K2 + extra, dtype=np.int32)
            before = order.copy()
            G = lib.wp_deal(_ptr(order), C.c_int64(len(order)), C.c_int64(K2), PB, C.c_int64(resident))
            assert G == min(-(-K2 // PB), resident)
            n = min(G * PB, K2)
            assert np.array_equal(np.sort(order[:n]), before[:n]) and np.array_equal(order[n:], before[n:])
            if n == G * PB:                                                            # every slot filled: slot b PB + pl holds entry pl G + b
                assert np.array_equal(order[:n].reshape(G, PB), before[:n].reshape(PB, G).T)
            else:                                                                      # ragged: the entries go in that order to the slots that exist
                slots = [b * PB + pl for pl in range(PB) for b in range(G) if b * PB + pl < n]
                assert np.array_equal(order[slots], before[:n])


def test_rows_form_geometry(lib, monkeypatch):
    def rows(K2, cus, slim, Ne, D, PB, CH):
        out = np.zeros(8, np.int64)
        lib.wp_rows(C.c_int64(K2), cus, slim, Ne, D, PB, CH, _ptr(out))
        return tuple(int(v) for v in out)

    def parked(D, PB, CH, budget):
        r = 1
        while r < 4096 and rows_lds(D, PB, CH, r + 1) <= budget:
            r += 1
        return r
    for setting, nt, budget in ((None, THREADS, LDS), ("1", THREADS, LDS), ("2", CU_THREADS, CU_LDS), ("3", 512, CU_LDS // 2)):
        if setting:
            monkeypatch.setenv("RVLL_WALK_ROWS", setting)
        for K2, cus, Ne, D in itertools.product((1, 63, 5000, 40000, 300000), (1, 256), (1, 200, 5000), (1, 19, 129)):
            assert rows(K2, cus, 0, Ne, D, 8, 4096)[:2] == (THREADS, LDS)              # the full solvers: the 256-thread form only
            got = rows(K2, cus, 1, Ne, D, 8, 4096)
            assert got[:2] == (nt, budget)
            if nt == THREADS:
                assert got[2:] == (1, 0, 0, 8, 4096, parked(D, 8, 4096, LDS))
                continue
            G = min(cus * (CU_THREADS // nt), K2)
            per = -(-K2 // G)
            ch = lambda sl: (max(sl * Ne, 3 * sl * D) + 1) & ~1                                      # noqa: E731
            slots = min(WAVE, per)
            while slots > 1 and rows_lds(D, slots, ch(slots), per) > budget:
                slots -= 1
            ok = rows_lds(D, slots, ch(slots), per) <= budget
            assert got[2:7] == (int(ok), G, per, slots, ch(slots)), (setting, K2, cus, Ne, D)
            if ok:
                assert got[7] == parked(D, slots, ch(slots), budget) >= per           # one launch takes every row
