"""CPU: the worker-thread pool behind the streamed host batches (evidence_amd/csrc/rvll_copypool.h) under ThreadSanitizer
and under AddressSanitizer + UBSan — the GPU box has no sanitizers, and the pool is plain C++."""
import os
import platform
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
SRC = REPO / "tests" / "native" / "copypool_main.cpp"


def _fixed_layout():
    """gcc's ThreadSanitizer expects the address-space layout it was built for; under a kernel with high-entropy ASLR a PIE
    binary can land outside it ("FATAL: ThreadSanitizer: unexpected memory mapping").  `setarch -R` turns randomisation off
    for the one process it starts, where the system allows that."""
    cmd = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") and subprocess.run(cmd + ["true"], capture_output=True).returncode == 0:
        return cmd
    return []


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_copy_pool_is_clean_under_sanitizers(tmp_path, sanitizer):
    exe = tmp_path / "copypool"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", f"-fsanitize={sanitizer}", "-fno-omit-frame-pointer",
           f"-I{REPO / 'evidence_amd' / 'csrc'}", str(SRC), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run(_fixed_layout() + [str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "copy pool run ok" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr and "ERROR" not in out.stderr
