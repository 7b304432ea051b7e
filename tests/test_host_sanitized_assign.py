"""The host side of lpf_assign_costs and lpf_assign_2d under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled
--offload-host-only and linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan
DRIVER=drive_assign`: the sanitized lpf_api object is built once per session and shared by every driver), driven by
tests/host_san/drive_assign.cpp: the refused arguments and their messages, host and device pointers, frames without rows or columns,
F = 0, every selection of outputs, the loop over frame ranges and no allocation on a second call of a shape."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_assign_host_side_under_asan_and_ubsan(tmp_path_factory):
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    b = subprocess.run(["make", "-C", SAN, "asan", "DRIVER=drive_assign", "OUT=" + out, "HIPCC=" + HIPCC], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "drive_assign_asan")], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_assign: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
