"""CPU: bench.py's launch path for N > 1, end to end through a stand-in model (tests/bench_stub.py) — the launcher
bench.py becomes when nobody launched it (VERDICT r2 missing #1), the externally launched form (RANK / WORLD_SIZE in
the environment, as `python -m torch.distributed.run` exports them), the one JSON line, the extras that cover
BASELINE.json configs[3] / configs[4], and what happens when a rank dies mid-phase (rank 0 reports what it
holds before it leaves)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np

from evidence_amd.synthetic import make_workload

REPO = Path(__file__).resolve().parents[1]
STUB = "tests.bench_stub:StubModel"


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RVLL_RDZV", "RVLL_RDZV_SECRET")}
    env.update(RVLL_BENCH_MODEL_FOR_TESTS=STUB, RVLL_PREWARM_S="0,0", PYTHONPATH=str(REPO), **extra)
    return env


def _run(args, **extra):
    r = subprocess.run([sys.executable, str(REPO / "bench.py")] + args, env=_env(**extra), capture_output=True, text=True,
                       timeout=300, cwd=str(REPO))
    lines = [json.loads(x) for x in r.stdout.strip().splitlines() if x.strip()]
    return r, lines


def test_bench_gpus_2_launches_itself_and_prints_one_line():
    r, lines = _run(["--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1                                   # ONE JSON line on stdout, whatever the ranks printed
    d = lines[0]
    assert d["n_gpus"] == 2 and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    cfg = d["config"]
    assert cfg["launched_by"] == "bench.py itself" and cfg["torch_in_process"] is False
    assert cfg["allgather"] == "host-socket-fallback" and "socket transport" in cfg["step_structure"]
    assert cfg["devices"] == [0, 0] and cfg["shared_device"] is True and "REHEARSAL" in d["data"]
    assert cfg["stub_model"] == STUB and "NOT a measurement" in d["data"]
    assert cfg["prewarm"]["launches"] >= 100 and "rule" in cfg["prewarm"]
    # the two BASELINE configurations that name 8 GPUs ride along as extras of the N > 1 line
    sc = d["sharded_configs"]
    assert sc["cfg4"]["live_points_total"] == 65536 and sc["cfg4"]["live_points_per_gpu"] == 32768 and sc["cfg4"]["evals_per_s"] > 0
    assert sc["cfg5"]["live_points_total"] == 131072 and sc["cfg5"]["live_points_per_gpu"] == 65536
    for prec in ("fp64", "mixed", "fp32"):
        assert sc["cfg5"][prec]["ms_per_step"] > 0
    assert 0 < sc["cfg5"]["fp32"]["max_rel_err_vs_fp64"] < 1e-6 and "max_rel_err_vs_fp64" not in sc["cfg5"]["fp64"]
    assert "extras_failed" not in d


def test_bench_under_an_external_launcher_meets_beside_master_port():
    """RANK / WORLD_SIZE / MASTER_* in the environment (torch.distributed.run's contract): no self-launch, the ranks meet
    on the abstract socket named after MASTER_ADDR / MASTER_PORT / run id."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(2):
        env = _env(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TORCHELASTIC_RUN_ID=f"t{os.getpid()}", RVLL_STUB_DEVICES="2")
        procs.append(subprocess.Popen([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1",
                                       "--no-cpu", "--no-extras"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, cwd=str(REPO)))
    outs = [p.communicate(timeout=300) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs[0][1][-2000:]
    assert outs[1][0].strip() == ""                          # only rank 0 prints
    d = json.loads(outs[0][0].strip())
    assert d["n_gpus"] == 2 and d["config"]["devices"] == [0, 1] and d["config"]["shared_device"] is False
    assert d["config"]["launched_by"].startswith("an external launcher") and "sharded_configs" not in d


def test_a_rank_that_dies_before_anything_was_measured_ends_the_run_with_a_line_that_says_so():
    # rank 1 leaves inside the socket transport's warm-up: rank 0 sees the peer go, prints the nothing-completed line
    # (value 0, which phase) and exits non-zero; the launcher relays the line and exits non-zero too
    r, lines = _run(["--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu"], RVLL_STUB_DIE_RANK="1", RVLL_STUB_DIE_AFTER="103")
    assert r.returncode != 0
    assert len(lines) == 1 and lines[0]["value"] == 0.0 and lines[0]["config"]["allgather"] == "rccl-hung"
    assert "socket transport" in lines[0]["config"]["hung_phase"] and "peer closed" in lines[0]["config"]["note"]
    assert "rank 1 exited with code 7" in r.stderr


def test_a_rank_that_dies_after_a_measurement_completed_does_not_take_that_line_with_it():
    """when a peer left first, rank 0 died of the launcher's SIGTERM or of a RendezvousError out of its next
    collective — without printing the verified line it already held.  Now it reports first."""
    r, lines = _run(["--gpus", "2", "--steps", "5", "--warmup", "2", "--no-cpu"], RVLL_STUB_DIE_RANK="1", RVLL_STUB_DIE_AFTER="118")
    assert len(lines) == 1 and lines[0]["value"] > 0 and lines[0]["n_gpus"] == 2
    assert "last completed measurement" in lines[0]["config"]["note"] and "sharded configs" in lines[0]["config"]["note"]
    assert r.returncode != 0                                 # a run in which a rank failed does not exit 0
    assert "rank 1 exited with code 7" in r.stderr


def test_bench_gpus_8_the_drivers_node_size():
    """The run the driver makes on an 8-GPU node and this pool cannot rehearse on hardware: eight ranks through
    the self-launcher and the rendezvous, ONE line, rc 0, the two BASELINE configurations that name 8 GPUs sharded as they
    name them — cfg4 8192 rows a rank, cfg5 16384."""
    r, lines = _run(["--gpus", "8", "--steps", "4", "--warmup", "1", "--no-cpu"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1
    d = lines[0]
    assert d["n_gpus"] == 8 and d["steps"] == 4 and d["scaling"] == "weak" and d["value"] > 0
    cfg = d["config"]
    assert cfg["devices"] == [0] * 8 and cfg["shared_device"] is True and cfg["launched_by"] == "bench.py itself"
    assert cfg["allgather"] == "host-socket-fallback" and cfg["torch_in_process"] is False
    sc = d["sharded_configs"]
    assert sc["cfg4"]["live_points_total"] == 65536 and sc["cfg4"]["live_points_per_gpu"] == 8192 and sc["cfg4"]["evals_per_s"] > 0
    assert sc["cfg5"]["live_points_total"] == 131072 and sc["cfg5"]["live_points_per_gpu"] == 16384
    for prec in ("fp64", "mixed", "fp32"):
        assert sc["cfg5"][prec]["ms_per_step"] > 0
    assert "extras_failed" not in d


def test_a_rank_of_eight_that_dies_mid_phase_does_not_take_the_line_with_it():
    # rank 5 of 8 leaves after the headline was measured and verified: the line still goes out (rank 0 reports first), rc != 0
    r, lines = _run(["--gpus", "8", "--steps", "4", "--warmup", "1", "--no-cpu"], RVLL_STUB_DIE_RANK="5", RVLL_STUB_DIE_AFTER="112")
    assert len(lines) == 1 and lines[0]["n_gpus"] == 8
    assert r.returncode != 0 and "rank 5 exited with code 7" in r.stderr
    if lines[0]["value"] > 0:
        assert "last completed measurement" in lines[0]["config"]["note"]
    else:
        assert lines[0]["config"]["allgather"] == "rccl-hung"


def test_bench_dump_outputs_writes_the_last_steps_log_l_the_same_from_run_to_run(tmp_path):
    """--dump-outputs DIR (N = 1): after the timed steps, logl.npy / flags.npy in float64 hold what the last step computed over
    the fixed, seeded live points; two runs with the same arguments write the same arrays."""
    dumps = []
    for run in ("a", "b"):
        r, lines = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-extras",
                         "--dump-outputs", str(tmp_path / run)])
        assert r.returncode == 0, r.stderr[-2000:]
        assert len(lines) == 1
        d = lines[0]
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["config"]["stub_model"] == STUB
        assert d["dumped_outputs"]["files"] == ["flags.npy", "logl.npy"] and d["dumped_outputs"]["sampled"] is False
        dumps.append({n: np.load(tmp_path / run / f"{n}.npy") for n in ("logl", "flags")})
    theta = make_workload(3).sample_theta(16384, seed=1234)
    assert np.array_equal(dumps[0]["logl"], -(theta * theta).sum(axis=1) - 1.0)        # the stub's stand-in for log-L
    for n, a in dumps[0].items():
        assert a.dtype == np.float64 and a.shape == (16384,) and np.array_equal(a, dumps[1][n])
