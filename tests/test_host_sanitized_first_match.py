"""lpf_first_match's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and
linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_first_match`:
the sanitized lpf_api object is built once per session and shared by every driver), driven by tests/host_san/drive_first_match.cpp:
the refused arguments and their messages, the camera it needs, host and device pointers for points, masks and outputs, several
selections of outputs, F = 0, M = 0, empty frames, the copies up and back of a host caller's lists, a repeated all-device call without
a host wait, and a batch larger than the staging bound, whose two ranges show in the recorded launch lines."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_first_match_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    b = subprocess.run(["make", "-C", SAN, "asan", "DRIVER=drive_first_match", "OUT=" + out, "HIPCC=" + HIPCC], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    trace = str(tmp_path / "launches.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", FAKE_HIP_TRACE=trace)
    r = subprocess.run([os.path.join(out, "drive_first_match_asan")], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_first_match: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    # the recorded launch lines: only this call's kernels, and the batch beyond the staging bound as ranges of 7 and 3 frames (two
    # tiles for the largest frame of each), then once more as one range with lent masks
    lines = [ln.split() for ln in open(trace).read().splitlines() if not ln.startswith(("copy", "memset"))]
    kernels = [(re.sub(r"^_Z\d+(lpf_fm_[a-z]+).*$", r"\1", ln[0]),) + tuple(int(x) for x in ln[1:]) for ln in lines]
    assert {k[0] for k in kernels} == {"lpf_fm_count", "lpf_fm_scan", "lpf_fm_scatter"}
    assert all(k[4:] == (256, 1, 1) for k in kernels)
    want = []
    for frames in (7, 3, 10):
        want += [("lpf_fm_count", 2, frames, 1), ("lpf_fm_scan", frames, 1, 1), ("lpf_fm_scatter", 2, frames, 1)]
    assert [k[:4] for k in kernels[-9:]] == want
    mangled = {ln[0] for ln in lines if "lpf_fm_count" in ln[0]}
    assert len(mangled) == 1                                   # (the driver's masks are uint8: one instance of the count kernel)
