"""lpf_first_match's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and
linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_first_match`:
the sanitized lpf_api object is built once per session and shared by every driver), driven by tests/host_san/drive_first_match.cpp:
the refused arguments and their messages, the camera it needs, host and device pointers for points, masks and outputs, several
selections of outputs, F = 0, M = 0, empty frames, the copies up and back of a host caller's lists, a repeated all-device call without
a host wait, and a batch larger than the staging bound, whose two ranges show in the recorded launch lines."""
import re

import host_san_run as san


@san.needs_hipcc
def test_first_match_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_first_match")
    text, every = san.drive(exe, trace=tmp_path / "launches.txt", checks=340)
    # the recorded launch lines: only this call's kernels, and the batch beyond the staging bound as ranges of 7 and 3 frames (two
    # tiles for the largest frame of each), then once more as one range with lent masks
    lines = [ln for ln in every if ln[0] not in ("copy", "memset")]
    kernels = [(re.sub(r"^_Z\d+(lpf_fm_[a-z]+).*$", r"\1", ln[0]),) + tuple(int(x) for x in ln[1:]) for ln in lines]
    assert {k[0] for k in kernels} == {"lpf_fm_count", "lpf_fm_scan", "lpf_fm_scatter"}
    assert all(k[4:] == (256, 1, 1) for k in kernels)
    want = []
    for frames in (7, 3, 10):
        want += [("lpf_fm_count", 2, frames, 1), ("lpf_fm_scan", frames, 1, 1), ("lpf_fm_scatter", 2, frames, 1)]
    assert [k[:4] for k in kernels[-9:]] == want
    mangled = {ln[0] for ln in lines if "lpf_fm_count" in ln[0]}
    assert len(mangled) == 1                                   # (the driver's masks are uint8: one instance of the count kernel)
