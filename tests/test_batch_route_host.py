"""CPU: which transport a host-buffer batch call takes and where its bytes lie (evidence_amd/csrc/rvll_batch_route.h: the routes
of rvll_loglike_batch, rvll_prior_batch and rvll_prior_loglike_batch, the layouts of the pinned result block and of a staging block,
the two chunk partitions — integer arithmetic), compiled alone for the host (tests/native/batchroute.cpp) and held against a second
statement of the rules in numpy.  Needs a host C++ compiler."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
SRC = HERE / "native" / "batchroute.cpp"
INC = HERE.parent / "evidence_amd" / "csrc"
PIN = 1 << 20
ZERO_COPY, PINNED_OUT, SPLIT, STREAMED, RESIDENT = range(5)          # Transport, in the header's order
LOGLIKE, PRIOR, PRIOR_LOGLIKE = range(3)
SWITCHES = ("RVLL_ZERO_COPY_IN_KB", "RVLL_STREAM_LOGLIKE", "RVLL_STREAM_MIN", "RVLL_SPLIT", "RVLL_NO_PINNED_OUT", "RVLL_STREAM_CHUNK",
            "RVLL_STREAM_LAG", "RVLL_STREAM_TIMING", "RVLL_COPY_THREADS")
SETTINGS = [{}, {"RVLL_SPLIT": "1"}, {"RVLL_SPLIT": "7"}, {"RVLL_NO_PINNED_OUT": "1"}, {"RVLL_STREAM_MIN": "1"},
            {"RVLL_STREAM_LOGLIKE": "1"}, {"RVLL_ZERO_COPY_IN_KB": "0"}]
NDIMS = (1, 2, 19, 74, 129)


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
    out = tmp_path_factory.mktemp("batchroute") / "libbatchroute.so"
    subprocess.run(cxx + ["-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror", f"-I{INC}", str(SRC), "-o", str(out)], check=True)
    return C.CDLL(str(out))


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _route(lib, entry, B, D, all_direct=True):
    out = np.zeros(5, np.int64)
    lib.br_route(C.c_int(entry), C.c_int64(B), C.c_int(D), C.c_int(all_direct), out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out)


def _stream_min(D, env):
    return max(1, int(env["RVLL_STREAM_MIN"])) if "RVLL_STREAM_MIN" in env else -(-(24 << 20) // (8 * D))


def _want(entry, B, D, env, all_direct=True):
    """(transport, nsplit, results through the pinned block, streamed chunk rows, lag): the rules, stated again."""
    nin, nout = 8 * B * D, 12 * B
    no_pin = "RVLL_NO_PINNED_OUT" in env
    split = max(1, min(64, int(env["RVLL_SPLIT"]))) if "RVLL_SPLIT" in env else None
    streamed = (STREAMED, 1, 0, 16384, 2)
    if entry == PRIOR:
        return (ZERO_COPY, 1, 1, 0, 0) if nin <= 384 * 1024 and not no_pin else (RESIDENT, 1, 0, 0, 0)
    if entry == LOGLIKE:
        zc = min(max(0, int(env["RVLL_ZERO_COPY_IN_KB"])) * 1024, PIN) if "RVLL_ZERO_COPY_IN_KB" in env else PIN
        pinned = int(nout <= PIN and not no_pin)
        if nin <= zc and nout <= PIN:
            return (ZERO_COPY, 1, 1, 0, 0)
        if "RVLL_STREAM_LOGLIKE" in env and B >= _stream_min(D, env):
            return streamed
        nsplit = min(8, max(2, B // 16384)) if B >= 16384 else 1
        nsplit = nsplit if split is None else split
        if nsplit > 1 and B >= 2 * nsplit:
            return (SPLIT, nsplit, pinned, 0, 0)
        return (PINNED_OUT if pinned else RESIDENT, 1, pinned, 0, 0)
    if nin + nout + 16 <= PIN and all_direct and not no_pin:
        return (ZERO_COPY, 1, 1, 0, 0)
    if B >= _stream_min(D, env):
        return streamed
    nsplit = 2 if 16384 <= B <= 131072 else 1
    nsplit = nsplit if split is None else split
    return (SPLIT, nsplit, 0, 0, 0) if nsplit > 1 and B >= 2 * nsplit else (RESIDENT, 1, 0, 0, 0)


def _sizes(D):
    """B = 1, 2 and one below, at and one above every row count at which some route begins or ends at D parameters"""
    edges = {PIN // (8 * D), PIN // 12, (384 * 1024) // (8 * D), (PIN - 16) // (8 * D + 12), -(-(24 << 20) // (8 * D)), 131072, 14, 128}
    edges.update(16384 * k for k in range(1, 10))
    edges.update(e + 1 for e in list(edges))             # ("up to n rows" and "from n + 1 rows on" are both edges)
    return sorted({1, 2} | {B for e in edges for B in (e - 1, e, e + 1) if B >= 1})


@pytest.mark.parametrize("env", SETTINGS, ids=lambda e: "-".join(f"{k[5:]}={v}" for k, v in e.items()) or "unset")
def test_routes_are_the_rules_at_every_threshold(lib, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    seen = set()
    for D in NDIMS:
        for B in _sizes(D):
            for entry in (LOGLIKE, PRIOR, PRIOR_LOGLIKE):
                got = _route(lib, entry, B, D)
                assert got == _want(entry, B, D, env), (entry, B, D, env)
                seen.add((entry, got[0]))
            assert _route(lib, PRIOR_LOGLIKE, B, D, all_direct=False) == _want(PRIOR_LOGLIKE, B, D, env, all_direct=False), (B, D, env)
    if not env:         # with no switch set, log-L is never streamed, and from 16384 rows on it is split, so never resident
        assert seen == {(LOGLIKE, ZERO_COPY), (LOGLIKE, PINNED_OUT), (LOGLIKE, SPLIT), (PRIOR, ZERO_COPY), (PRIOR, RESIDENT),
                        (PRIOR_LOGLIKE, ZERO_COPY), (PRIOR_LOGLIKE, SPLIT), (PRIOR_LOGLIKE, STREAMED), (PRIOR_LOGLIKE, RESIDENT)}
    if "RVLL_STREAM_LOGLIKE" in env:
        assert (LOGLIKE, STREAMED) in seen


def test_the_row_counts_the_source_comments_quote_at_19_parameters(lib):
    D = 19
    assert _route(lib, LOGLIKE, 6898, D)[0] == ZERO_COPY and _route(lib, LOGLIKE, 6899, D)[0] == PINNED_OUT
    assert _route(lib, PRIOR, 2586, D)[0] == ZERO_COPY and _route(lib, PRIOR, 2587, D)[0] == RESIDENT
    assert _route(lib, PRIOR_LOGLIKE, 6393, D)[0] == ZERO_COPY and _route(lib, PRIOR_LOGLIKE, 6394, D)[0] == RESIDENT
    for ndim in NDIMS:                                   # results through the pinned block: up to 87381 rows at any ndim
        assert _route(lib, LOGLIKE, 87381, ndim)[2] == 1 and _route(lib, LOGLIKE, 87382, ndim)[2] == 0
    assert _route(lib, PRIOR_LOGLIKE, 165564, D)[0] == RESIDENT and _route(lib, PRIOR_LOGLIKE, 165565, D) == (STREAMED, 1, 0, 16384, 2)


def test_switches_are_read_with_their_clamps(lib, monkeypatch):
    def read():
        out = np.zeros(9, np.int64)
        lib.br_switches(out.ctypes.data_as(C.c_void_p))
        return out.tolist()
    assert read() == [PIN, 0, 0, 0, 0, 16384, 2, 0, 0]
    for name, value in zip(SWITCHES, ("64", "", "5000", "99", "1", "100", "7", "1", "40")):
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("RVLL_SPLITS", "3")               # another name that begins like a switch's
    assert read() == [64 * 1024, 1, 5000, 64, 1, 256, 2, 1, 32]
    for name, value in (("RVLL_ZERO_COPY_IN_KB", "4096"), ("RVLL_STREAM_MIN", "0"), ("RVLL_SPLIT", "0"), ("RVLL_STREAM_LAG", "0"),
                        ("RVLL_STREAM_CHUNK", "30000"), ("RVLL_COPY_THREADS", "0")):
        monkeypatch.setenv(name, value)
    assert read() == [PIN, 1, 1, 1, 1, 30000, 1, 1, 1]


def test_download_routes(lib):
    PINNED, DIRECT, STAGED = range(3)
    for D in NDIMS:
        for B in _sizes(D) + [(32 << 20) // (8 * D) + k for k in (-1, 0, 1, 2)]:
            for theta, logl, flags in ((1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0)):
                nt, rest = 8 * B * D * theta, 8 * B * logl + 4 * B * flags
                want = PINNED if nt + rest <= PIN else STAGED if nt >= 32 << 20 else DIRECT
                assert lib.br_download(C.c_int64(B), C.c_int(D), theta, logl, flags) == want, (B, D, theta, logl, flags)
    assert lib.br_download(C.c_int64(56679), 74, 1, 0, 0) == DIRECT and lib.br_download(C.c_int64(56680), 74, 1, 0, 0) == STAGED


@pytest.mark.parametrize("D", [1, 19, 74])
def test_pinned_result_block_of_every_size_a_route_admits(lib, D):
    def blocks(nmax):
        out = np.zeros((nmax, 3), np.int64)
        lib.br_pinned_results(C.c_int64(nmax), out.ctypes.data_as(C.c_void_p))
        return out.T
    nmax = PIN // 12                                      # log-L and flags alone: every route whose results leave through the block
    assert _route(lib, LOGLIKE, nmax, D)[2] == 1 and _route(lib, LOGLIKE, nmax + 1, D)[2] == 0
    B = np.arange(1, nmax + 1)
    logl, flags, _ = blocks(nmax)
    assert (logl == 0).all() and (flags == 8 * B).all() and (flags + 4 * B <= PIN).all()    # B doubles, then B ints, inside the block
    nmax = (PIN - 16) // (8 * D + 12)                     # with theta: the fused zero-copy route
    assert _route(lib, PRIOR_LOGLIKE, nmax, D)[0] == ZERO_COPY and _route(lib, PRIOR_LOGLIKE, nmax + 1, D)[0] != ZERO_COPY
    B = np.arange(1, nmax + 1)
    logl, flags, theta = blocks(nmax)
    assert (logl == 0).all() and (flags == logl + 8 * B).all()                      # log-L ends where the flags begin ...
    assert (theta >= flags + 4 * B).all() and (theta < flags + 4 * B + 16).all() and (theta % 16 == 0).all()   # ... theta behind them
    assert (theta + 8 * B * D <= PIN).all()                                         # ... and its B D doubles end inside the block


def test_staging_block_layout(lib):
    for rows, D in ((256, 1), (4096, 19), (16384, 19), (30000, 74), (16384, 129)):
        out = np.zeros(5, np.int64)
        lib.br_stage_block(C.c_int64(rows), C.c_int(D), out.ctypes.data_as(C.c_void_p))
        assert out.tolist() == [8 * rows * D, 0, 8 * rows * D, 8 * rows * (D + 1), 8 * rows * (D + 1) + 4 * rows]


def _covers(chunks, B):
    """chunks [n, 2] cover [0, B) exactly once, in order, none empty"""
    return chunks[0, 0] == 0 and chunks[-1, 1] == B and (chunks[1:, 0] == chunks[:-1, 1]).all() and (chunks[:, 1] > chunks[:, 0]).all()


def test_both_chunk_partitions_cover_every_row_once(lib):
    for nsplit in (2, 3, 7, 8, 64):
        for B in (2 * nsplit, 2 * nsplit + 1, 16384, 40001, 131071, 131072, 230_001):       # B == 2 nsplit: the least the route takes
            out = np.zeros((nsplit, 2), np.int64)
            lib.br_split_chunks(C.c_int64(B), C.c_int(nsplit), out.ctypes.data_as(C.c_void_p))
            assert _covers(out, B), (B, nsplit)
            assert (out[:, 0] == B * np.arange(nsplit) // nsplit).all()
    for rows in (256, 4096, 16384, 30000):
        for B in (1, 3, rows - 1, rows, rows + 1, 2 * rows, 2 * rows + 7, 70_000, 230_001):  # fewer rows than a chunk, fewer chunks
            out = np.zeros((B // rows + 2, 2), np.int64)                                    # than the pipeline is deep, ragged ends
            n = lib.br_stream_chunks(C.c_int64(B), C.c_int64(rows), C.c_int(len(out)), out.ctypes.data_as(C.c_void_p))
            assert n == -(-B // rows) and _covers(out[:n], B), (B, rows)
            assert (out[:n - 1, 1] - out[:n - 1, 0] == rows).all() and out[n - 1, 1] - out[n - 1, 0] <= rows
