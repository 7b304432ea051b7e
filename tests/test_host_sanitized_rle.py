"""lpf_set_masks_rle's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and linked
against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_rle`: the sanitized
lpf_api object is built once per session and shared by every driver), driven by tests/host_san/drive_rle.cpp -- a stand-alone program:
every refusal with its message (start = length = INT32_MAX, run_off[0] = 1 and a run_off that decreases among them) and nothing queued
by any, the state errors (no camera, inside a capture), F = 0 / M = 0 / no runs without a decode launch, erode_iters = 2 as decode + 2
erosions, 10^5 runs, growing then shrinking calls, the pipelined modes, and the caller's arrays freed right after each call.  The fake
runtime's launch trace tells which kernels ran."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_set_masks_rle_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    out = str(tmp_path_factory.getbasetemp() / "host_san")
    b = subprocess.run(["make", "-C", SAN, "asan", "DRIVER=drive_rle", "OUT=" + out, "HIPCC=" + HIPCC], capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, (b.stdout + b.stderr)[-3000:]
    trace = str(tmp_path / "launches.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1", FAKE_HIP_TRACE=trace)
    r = subprocess.run([os.path.join(out, "drive_rle_asan")], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_rle: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    with open(trace) as f:
        lines = [line.split() for line in f if line.strip() and line.split()[0] not in ("copy", "memset")]
    names = [l[0] for l in lines]
    decodes = [l for l in lines if "lpf_rle_decode" in l[0]]
    # the three label element widths were decoded, by blocks of 256 threads
    for lt in ("IhE", "ItE", "IjE"):
        assert any(lt in d[0] for d in decodes), lt
    assert all(d[4:] == ["256", "1", "1"] for d in decodes)
    # the full-image run at 1408 x 376: 517 units of 1024 pixels, four per block
    assert any(d[1] == str((-(-1408 * 376 // 1024) + 3) // 4) for d in decodes)
    # erosion after a decode is the packed image's: the cross and the k x k element, never a pack with a fused first iteration
    i = next(k for k, n in enumerate(names) if "lpf_rle_decode" in n and k + 2 < len(names) and "lpf_erode_packed" in names[k + 1])
    assert "lpf_erode_packed" in names[i + 1] and "lpf_erode_packed" in names[i + 2]
    assert any("lpf_erode_packed_k" in n for n in names)
    assert not any("lpf_pack_erode_k" in n for n in names)
