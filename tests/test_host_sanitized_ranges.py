"""The host side of the nine batched analysis calls under AddressSanitizer + UndefinedBehaviorSanitizer with tiny ranges: lpf_api.hip
compiled --offload-host-only with -DLPF_LAB (tests/host_san/Makefile's EXTRA: the object has a name of its own and does not replace
the plain one the other drivers share) and linked against tests/host_san/fake_hip.cpp, driven by tests/host_san/drive_ranges.cpp.
lpf_lab_set_range_limits cuts batches of six items into ranges of one and of two and by a budget of one byte, so every call's
staging spans run over real heap bounds range after range; the driver checks return codes, lpf_lab_last_ranges and the launches of
every range.  A stand-alone program: nothing is preloaded, nothing loaded into Python is sanitized."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_batched_calls_in_tiny_ranges_under_asan_and_ubsan(tmp_path_factory):
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    b = subprocess.run(["make", "-C", SAN, "asan", "DRIVER=drive_ranges", "EXTRA=-DLPF_LAB", "OUT=" + out, "HIPCC=" + HIPCC],
                       capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    assert os.path.exists(os.path.join(out, "lpf_api_LPF_LAB_asan.o"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(out, "drive_ranges_asan")], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_ranges: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
