"""Sanitizers for the code that runs on the host ("race detection / sanitizers"; build container only -- never on a
GPU box, where sanitizer runs are not available):

  * oracle/lpf_oracle.c under AddressSanitizer + UndefinedBehaviorSanitizer (`make -C oracle asan`), running the oracle's own
    golden-vector and mask tests against the sanitized library;
  * the HOST side of liblpf -- lpf_api.hip compiled `--offload-host-only` and linked against tests/host_san/fake_hip.cpp, a functional
    stand-in for the HIP runtime (device memory = heap blocks, copies = memcpy, launches = nothing) -- under ASan + UBSan and under
    ThreadSanitizer, driven by tests/host_san/drive.cpp: argument validation, host-memory runs, lpf_run_cams / lpf_run_cams_wide /
    lpf_run_wide / lpf_run_frame_wide / lpf_depth_maps with host and device outputs, > 24 000 software-pipelined runs with
    new masks / rectangles / boxes / batch shapes (the pinned upload ring is lapped many times, with pieces that fill a quarter
    exactly: ADVICE round 3), the box-set and scratch-set rotation, the graph state machine, and the reader's worker threads; then
    every source a run's tiles take their label bits from -- uint8 masks and float masks under each rule, from host memory, copied and
    lent device memory, aligned or not, M = 0 / 5 / 12 / 32, with and without rectangles and erosion, serial, mode 2 and mode 4, in
    small sparse, small dense, large dense and (14 frames and more of 1408 x 376) large sparse launches, with and without a box job,
    through device and host memory; a mode switch, a camera of another size, a label image read or set, masks for no frames and a
    graph capture with unpacked masks pending; mode-4 launches whose pack and tiles do not go together; and the packs of
    lpf_run_cams / lpf_run_wide / lpf_depth_maps for every rule and label width.  fake_hip.cpp records every launch (kernel name,
    grid, block) and every copy and memset (kind, bytes): the driver prints the launch count and hash and the hash of the copies per
    section, and FAKE_HIP_TRACE=<file> keeps the lines.
"""
import os
import subprocess
import sys

import pytest

import host_san_run as san

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gcc_lib(name):
    p = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return p if os.path.isabs(p) and os.path.exists(p) else None


@pytest.mark.skipif(_gcc_lib("libasan.so") is None, reason="gcc's libasan is not installed")
def test_oracle_under_asan_and_ubsan():
    subprocess.check_call(["make", "-C", os.path.join(REPO, "oracle"), "-s", "asan"])
    env = dict(os.environ, LD_PRELOAD=_gcc_lib("libasan.so"), ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               LPF_ORACLE_SO=os.path.join(REPO, "oracle", "liblpf_oracle_asan.so"))
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_oracle_golden.py", "tests/test_oracle_masks.py", "-q", "-x", "-p", "no:cacheprovider"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and " passed" in text, text[-3000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]


@san.needs_hipcc
@pytest.mark.parametrize("san_name", ["asan", "tsan"])
def test_host_side_of_the_library_under_sanitizers(tmp_path, tmp_path_factory, san_name):
    exe = san.build(tmp_path_factory, "drive", san_name)          # (one build directory for every driver: one lpf_api object per sanitizer)
    scans = tmp_path / "scans"
    scans.mkdir()
    san.drive(exe, scans, 12000, checks=208276)                 # (the count repeats from run to run, under both sanitizers)
