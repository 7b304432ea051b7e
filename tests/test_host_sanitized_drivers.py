"""The host side of the batched analysis calls under AddressSanitizer + UndefinedBehaviorSanitizer, one stand-alone driver per call:
lpf_api.hip compiled --offload-host-only and linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by
tests/host_san/Makefile (`make asan DRIVER=<driver>`: the sanitized lpf_api object is built once per session and EXTRA and shared by
every driver), built and run by tests/host_san_run.py.  Each driver's head comment says in full what it drives; kernel launches do
nothing there, the values are checked by the GPU tests.  The drivers whose launch trace a test reads have test files of their own."""
import os

import pytest

import host_san_run as san

# driver, EXTRA, CHECKs it evaluates, what it covers
DRIVERS = [
    ("drive_inside", None, 28588, "lpf_inside_masks: refusals and messages, the boxes it needs in force, host and device pointers for points, "
     "lists and outputs, NULL outputs, M = 0, F = 0, a frame whose lists did not fit, the copies back to a host caller"),
    ("drive_match2d", None, 105, "lpf_match_2d: refusals and messages, host and device pointers, frames without detections or boxes, F = 0, "
     "the loop over frame ranges"),
    ("drive_box_views", None, 133, "lpf_box_views: refusals and messages, host and device pointers, frames without boxes, F = 0, every "
     "selection of outputs, the loop over frame ranges"),
    ("drive_box_points", None, 2155, "lpf_box_points: refusals and messages, the boxes it needs in force, host and device pointers, NULL "
     "outputs in every combination, LW = 0 and NULL labels, F = 0, frames without valid points or boxes, the checks of host lists, the "
     "copies back to a host caller, a repeated all-device call without a host wait"),
    ("drive_overlays", None, 65, "lpf_depth_overlays: refusals and messages, host and device pointers, the chunk loop"),
    ("drive_assign", None, 294, "lpf_assign_costs and lpf_assign_2d: refusals and messages, host and device pointers, frames without rows "
     "or columns, F = 0, every selection of outputs, the loop over frame ranges, no allocation on a second call of a shape"),
    ("drive_ranges", "-DLPF_LAB", 196, "the nine batched analysis calls in tiny ranges: lpf_lab_set_range_limits cuts batches of six items "
     "into ranges of one and of two and by a budget of one byte, so every call's staging spans run over real heap bounds range after "
     "range; return codes, lpf_lab_last_ranges and the launches of every range (the lab build's object has a name of its own and does "
     "not replace the plain one the other drivers share)"),
]


@san.needs_hipcc
@pytest.mark.parametrize("driver,extra,checks,covers", DRIVERS, ids=[d[0] for d in DRIVERS])
def test_driver_under_asan_and_ubsan(tmp_path_factory, driver, extra, checks, covers):
    exe = san.build(tmp_path_factory, driver, extra=extra)
    if extra:
        assert os.path.exists(os.path.join(os.path.dirname(exe), "lpf_api_%s_asan.o" % extra[2:]))
    san.drive(exe, checks=checks)
