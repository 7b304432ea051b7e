"""lpf_inside_masks's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and
linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime), with the commands of tests/host_san/Makefile, driven by
tests/host_san/drive_inside.cpp: the refused arguments and their messages, the boxes it needs in force, host and device pointers for
points, lists and outputs, NULL outputs, M = 0, F = 0, a frame whose lists did not fit, and the copies back to a host caller."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SAN = os.path.join(REPO, "tests", "host_san")
CSRC = os.path.join(REPO, "lidar_object_detection_amd", "csrc")
COMMON = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off"]
FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")
def test_inside_masks_host_side_under_asan_and_ubsan(tmp_path):
    out = str(tmp_path)

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=SAN)
        assert r.returncode == 0, (" ".join(cmd) + "\n" + r.stdout + r.stderr)[-3000:]
        return r.stdout
    api_o = os.path.join(out, "lpf_api.o")
    run([HIPCC, "--offload-host-only"] + COMMON + FLAGS + ["-c", os.path.join(CSRC, "lpf_api.hip"), "-o", api_o])
    syms = [l.split()[-1] for l in run(["nm", "-u", api_o]).splitlines() if "__hip_fatbin_" in l]
    fat_c = os.path.join(out, "fatbin.c")
    with open(fat_c, "w") as f:
        f.write("".join("const char %s[64] = {0};\n" % s for s in syms))
    objs = [api_o]
    for src in ("fake_hip.cpp", "drive_inside.cpp"):
        o = os.path.join(out, src + ".o")
        run([HIPCC, "--offload-host-only"] + COMMON + FLAGS + ["-x", "c++", "-c", os.path.join(SAN, src), "-o", o])
        objs.append(o)
    run(["gcc", "-c", fat_c, "-o", os.path.join(out, "fatbin.o")])
    exe = os.path.join(out, "drive_inside")
    run(["/opt/rocm/lib/llvm/bin/clang++"] + FLAGS + objs + [os.path.join(out, "fatbin.o"), "-pthread", "-ldl", "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=env)
    text = r.stdout + r.stderr
    assert r.returncode == 0 and "drive_inside: 0 failed checks" in text, text[-4000:]
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
