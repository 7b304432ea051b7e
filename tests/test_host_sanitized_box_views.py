"""lpf_box_views' host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and
linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_box_views`:
the sanitized lpf_api object is built once per session and shared by every driver), driven by
tests/host_san/drive_box_views.cpp: the refused arguments and their messages, host and device pointers, frames without boxes, F = 0,
every selection of outputs and the loop over frame ranges."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_box_views_host_side_under_asan_and_ubsan(tmp_path_factory):
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    b = subprocess.run(["make", "-C", SAN, "asan", "DRIVER=drive_box_views", "OUT=" + out, "HIPCC=" + HIPCC], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "drive_box_views_asan")], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_box_views: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
