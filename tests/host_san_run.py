"""Builds and runs the stand-alone sanitizer drivers of tests/host_san (drive*.cpp: lpf_api.hip compiled --offload-host-only and linked
against fake_hip.cpp, the stand-in HIP runtime) for the tests/test_host_sanitized*.py files.  A plain module: the tests import what they
use.  The drivers are programs of their own, run as child processes on the CPU; nothing is preloaded and nothing loaded into Python is
sanitized here."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


def build(tmp_path_factory, driver, san="asan", extra=None):
    """`make <san> DRIVER=<driver> [EXTRA=<extra>]` into the session's one build directory (the sanitized lpf_api object is built once per
    sanitizer and EXTRA, and shared by every driver of the session); returns the executable's path."""
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    cmd = ["make", "-C", SAN, san, "DRIVER=" + driver, "OUT=" + out, "HIPCC=" + HIPCC]
    if extra:
        cmd.append("EXTRA=" + extra)
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    return os.path.join(out, "%s_%s" % (driver, san))


def drive(exe, *args, trace=None, checks=None):
    """Runs a driver: it must end with status 0, report no failed check and leave the sanitizers silent; checks=N: it must have evaluated
    N CHECKs.  Returns its output, and with trace=<path> (FAKE_HIP_TRACE) also the trace file's lines, split."""
    name = os.path.basename(exe).rsplit("_", 1)[0]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", TSAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    if trace is not None:
        env["FAKE_HIP_TRACE"] = str(trace)
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and name + ": 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    if checks is not None:
        assert re.search(r"^%s: .*, %d checks run$" % (re.escape(name), checks), text, re.M), text[-400:]
    if trace is None:
        return text
    with open(trace) as f:
        return text, [line.split() for line in f if line.strip()]
