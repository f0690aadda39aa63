"""CPU: the walker groups of a resident ensemble step (evidence_amd/csrc/rvll_step_groups.h: stages 3 and 5 of DESIGN §4e, pure
index arithmetic) compiled for the host (tests/native/stepgroups.cpp) against nested._walk_groups and a direct numpy statement of
the segment table and the groups' survivors; and the same code once as a program under the address and undefined-behaviour
sanitizers.  Needs a host C++ compiler."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from evidence_amd.nested import _GROUP_MUL, _M64, _walk_groups

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "stepgroups.cpp"
INC = HERE.parent / "evidence_amd" / "csrc"
A, KDEAD, M, D = 3, 7, 20, 2


def _compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return [shutil.which(name)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return [hipcc, "-x", "c++"] if Path(hipcc).exists() else None


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("stepgroups")
    common = ["-std=c++17", "-Wall", "-Werror", f"-I{INC}", str(SRC)]
    subprocess.run(cxx + ["-O2", "-fPIC", "-shared"] + common + ["-o", str(out / "libstepgroups.so")], check=True)
    subprocess.run(cxx + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSTEPGROUPS_MAIN"] + common
                   + ["-o", str(out / "stepgroups_san")], check=True)
    return C.CDLL(str(out / "libstepgroups.so")), out / "stepgroups_san", out


def _labels(rng, sizes):
    """m labels: cluster c on sizes[c] rows, in a random arrangement"""
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def _cases():
    """(lab [A, m], ncl [A], ranks [A, kdead], lstar [A], seeds [A], steps [A] or None, nsteps).  Every case has runs of 1, 2 and 4
    clusters: the run with one takes no segment at all; of the run with four, cluster 1 (3 rows < 2 D) and cluster 3 (2 rows) take
    none, and no walker starts in cluster 3.  Seeds up to 2^64 so that seed + c _GROUP_MUL wraps."""
    rng = np.random.default_rng(20)
    out = []
    for k, steps in enumerate((None, [5, 9, 3], [4, 4, 4], [1, 7, 7])):
        sizes = [[M], [12, 8], [10, 3, 5, 2]]
        order = rng.permutation(3)
        lab = np.stack([_labels(rng, sizes[i]) for i in order])
        ncl = np.array([len(sizes[i]) for i in order], dtype=np.int32)
        ranks = np.empty((A, KDEAD), dtype=np.int32)
        for a in range(A):
            allowed = np.flatnonzero(lab[a] != 3)
            ranks[a] = rng.choice(allowed, KDEAD)
            started = [c for c in range(ncl[a]) if c != 3]                              # ... and one in each of the others
            ranks[a, :len(started)] = [np.flatnonzero(lab[a] == c)[0] for c in started]
        lstar = rng.normal(-50.0, 5.0, A)
        seeds = rng.integers(0, 2 ** 64, A, dtype=np.uint64)
        if k == 1:
            seeds[:] = 2 ** 64 - 1 - np.arange(A, dtype=np.uint64)
        out.append((lab, ncl, ranks, lstar, seeds, None if steps is None else np.array(steps, dtype=np.int32), 11))
    return out


def _bad_cases():
    lab, ncl, ranks, lstar, seeds, steps, nsteps = _cases()[0]
    a4 = int(np.flatnonzero(ncl == 4)[0])
    a2 = int(np.flatnonzero(ncl == 2)[0])
    out = []
    for run, value in ((a4, 4), (a2, -1), (a2, 2)):                       # a label at the count, below 0, beyond a smaller count
        bad = lab.copy()
        bad[run, 13] = value
        out.append(((bad, ncl, ranks, lstar, seeds, steps, nsteps), (2, run, value)))
    for run, value in ((1, 0), (2, M + 1), (0, -3)):                      # a cluster count of 0, above m, negative
        bad = ncl.copy()
        bad[run] = value
        out.append(((lab, bad, ranks, lstar, seeds, steps, nsteps), (1, run, value)))
    return out


def _expected(lab, ncl, ranks, lstar, seeds, steps, nsteps):
    """The same tables from numpy and nested._walk_groups."""
    cnt = [np.bincount(lab[a], minlength=ncl[a]) for a in range(A)]
    segtab, segsc, seg_of = [], [], []
    for a in range(A):
        if ncl[a] == 1:
            continue
        off = a * M + np.concatenate([[0], np.cumsum(cnt[a])[:-1]])
        for c in range(ncl[a]):
            if cnt[a][c] >= 2 * D:
                segtab += [int(off[c]), int(cnt[a][c])]
                segsc += [1.0 / cnt[a][c], 1.0 / (cnt[a][c] - 1)]
                seg_of += [a, c]
    perm, grun, grid, gofs, gcnt, glstar, gseed, gsteps, gfac = [], [], [], [], [], [], [], [], []
    for a in range(A):
        wo, sizes, clusters, gseeds = _walk_groups(lab[a][ranks[a]].astype(np.intp), list(range(ncl[a])), int(seeds[a]))
        perm += list(a * KDEAD + wo)
        off = a * M + np.concatenate([[0], np.cumsum(cnt[a])[:-1]])
        for c, size, s in zip(clusters, sizes, gseeds):
            grun += [len(gofs)] * int(size)
            grid += list(range(int(size)))
            gofs.append(int(off[c])); gcnt.append(int(cnt[a][c])); glstar.append(float(lstar[a])); gseed.append(int(s))
            gsteps.append(int(steps[a]) if steps is not None else nsteps); gfac += [a, int(c)]
            assert s == (int(seeds[a]) if c == 0 else (int(seeds[a]) + int(c) * _GROUP_MUL) & _M64)
    cflat = np.full((A, M), -1, dtype=np.int64)
    for a in range(A):
        cflat[a, :ncl[a]] = cnt[a]
    return dict(cnt=cflat.ravel().tolist(), segtab=segtab, segsc=segsc, seg_of=seg_of, perm=[int(v) for v in perm], grun=grun, grid=grid,
                gofs=gofs, gcnt=gcnt, glstar=glstar, gseed=gseed, gsteps=gsteps, gfac=gfac)


def _call(lib, lab, ncl, ranks, lstar, seeds, steps, nsteps):
    K, N = A * KDEAD, A * M
    i32, i64, f64, u64 = np.int32, np.int64, np.float64, np.uint64
    o = dict(sizes=np.zeros(2, i64), cnt=np.zeros(N, i64), segtab=np.zeros(2 * N, i64), segsc=np.zeros(2 * N, f64), seg_of=np.zeros(2 * N, i32),
             perm=np.zeros(K, i32), grun=np.zeros(K, i32), grid=np.zeros(K, i32), gofs=np.zeros(K, i64), gcnt=np.zeros(K, i64),
             glstar=np.zeros(K, f64), gseed=np.zeros(K, u64), gsteps=np.zeros(K, i32), gfac=np.zeros(2 * K, i32))
    ins = [np.ascontiguousarray(lab, i32), np.ascontiguousarray(ncl, i32), np.ascontiguousarray(ranks, i32), np.ascontiguousarray(lstar, f64),
           np.ascontiguousarray(seeds, u64)]
    st = None if steps is None else np.ascontiguousarray(steps, i32)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = lib.sg_build(*[ptr(x) for x in ins], None if st is None else ptr(st), C.c_int32(nsteps), C.c_int32(A), C.c_int64(KDEAD), C.c_int64(M),
                      C.c_int32(D), *[ptr(x) for x in o.values()])
    S, G = (int(v) for v in o["sizes"])
    if rc:
        return rc, S, G, None
    n = dict(cnt=N, segtab=2 * S, segsc=2 * S, seg_of=2 * S, perm=K, grun=K, grid=K, gofs=G, gcnt=G, glstar=G, gseed=G, gsteps=G, gfac=2 * G)
    return rc, S, G, {k: o[k][:n[k]].tolist() for k in n}


def test_cases_hold_what_they_are_meant_to():
    nonuniform = 0
    for lab, ncl, ranks, lstar, seeds, steps, nsteps in _cases():
        assert sorted(ncl) == [1, 2, 4]
        a = int(np.flatnonzero(ncl == 4)[0])
        cnt, started = np.bincount(lab[a], minlength=4), np.bincount(lab[a][ranks[a]], minlength=4)
        assert started[3] == 0 and (started[:3] > 0).all()                      # a cluster no walker starts in
        assert 0 < cnt[1] < 2 * D and 0 < cnt[3] < 2 * D and cnt[0] >= 2 * D    # clusters that take no segment
        nonuniform += steps is not None and len(set(steps.tolist())) > 1
    assert nonuniform >= 1


def test_groups_and_segments_are_numpys_and_walk_groups(built):
    lib = built[0]
    for case in _cases():
        rc, S, G, got = _call(lib, *case)
        want = _expected(*case)
        assert rc == 0 and S == len(want["seg_of"]) // 2 and G == len(want["gofs"])
        assert S == 4 and G == 1 + 2 + 3              # (2 + 2 clusters of at least 2 D rows; every cluster but the empty one)
        for key in want:
            assert got[key] == want[key], key


def test_bad_labels_and_cluster_counts_are_reported_not_indexed(built):
    lib = built[0]
    for case, (what, run, value) in _bad_cases():
        rc, bad_run, bad_value, _ = _call(lib, *case)
        assert (rc, bad_run, bad_value) == (what, run, value)


def _case_text(lab, ncl, ranks, lstar, seeds, steps, nsteps):
    lines = [f"{A} {KDEAD} {M} {D} {nsteps} {int(steps is not None)}", " ".join(map(str, lab.ravel())), " ".join(map(str, ncl)),
             " ".join(map(str, ranks.ravel())), " ".join(float(v).hex() for v in lstar), " ".join(str(int(v)) for v in seeds)]
    if steps is not None:
        lines.append(" ".join(map(str, steps)))
    return "\n".join(lines) + "\n"


def test_the_same_cases_under_the_sanitizers(built):
    """A stand-alone program of the same wrapper, built with -fsanitize=address,undefined: it ends clean on every case, the refused
    ones included, and prints the tables the library build returned."""
    lib, prog, out = built
    cases = _cases() + [c for c, _ in _bad_cases()]
    (out / "cases.txt").write_text("".join(_case_text(*c) for c in cases))
    run = subprocess.run([str(prog), str(out / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = iter(run.stdout.split("\n"))
    keys = ("cnt", "segtab", "segsc", "seg_of", "perm", "grun", "grid", "gofs", "gcnt", "glstar", "gseed", "gsteps", "gfac")
    for case in cases:
        rc, s0, s1, want = _call(lib, *case)
        assert [int(v) for v in next(lines).split()] == [rc, s0, s1]
        if rc:
            continue
        for key in keys:
            conv = float.fromhex if key in ("segsc", "glstar") else int
            assert [conv(v) for v in next(lines).split()] == want[key], key
    assert [ln for ln in lines if ln.strip()] == []
