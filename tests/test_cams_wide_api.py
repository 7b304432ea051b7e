"""The multi-camera wide entry point (lpf_run_cams_wide) without a GPU: the header declares it, the library's export list names it,
and the Python entries refuse bad arguments before anything reaches the GPU."""
import re

import numpy as np
import pytest

from lidar_object_detection_amd import _native, pipeline
from test_multicam_api import HEADER, _Camera, _cam, _NoGpu


def test_header_declares_the_multicam_wide_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+lpf_run_cams_wide\s*\(([^;]*)\)\s*;", text)
    assert m, "lpf_run_cams_wide is not declared"
    args = " ".join(m.group(1).split())
    assert "const lpf_cam_input *cams, int C" in args and "const lpf_wide_outputs *out" in args, args
    assert re.search(r"#define\s+LPF_MAX_MASKS_WIDE\s+256\b", raw)
    assert "lpf_run_cams_wide" in _native.EXPORTED
    assert hasattr(_native.LpfContext, "run_cams_wide")


def _u8(M, F=None, H=48, W=64):
    return np.zeros((M, H, W) if F is None else (F, M, H, W), np.uint8)


@pytest.mark.parametrize("cams", [
    [],                                                                      # C = 0
    [_cam() for _ in range(5)],                                              # C = 5
    [_cam(_u8(257))],                                                        # M = 257: above LPF_MAX_MASKS_WIDE
    [_cam(_u8(40)), _cam(_u8(257))],                                         # ... in the second camera
    [_cam(_u8(40)), _cam(np.zeros((40, 48, 63), np.uint8))],                 # not camera 1's size
    [_cam(np.zeros((40, 40, 30), np.uint8), W=30, H=41)],                    # not this camera's size either
    [_cam(_u8(40, F=2))],                                                    # two frames of masks for one frame of points
    [_cam(np.zeros((40, 48), np.uint8))],                                    # not [M,H,W]
    [_cam(_u8(40), binarize="round")],
    [_cam(_u8(40), erode_iters=-1)],
    [_cam(_u8(40), rects=np.zeros((39, 4), np.int32))],
    [_cam(_u8(40), boxes=[np.zeros((1, 8, 3)), np.zeros((1, 8, 3))])],      # boxes for two frames
])
def test_run_cams_wide_refuses_bad_arguments_before_the_gpu(cams):
    ctx = _NoGpu()
    with pytest.raises(ValueError):
        ctx.run_cams_wide([np.zeros((10, 4), np.float32)], cams)


def test_run_cams_wide_takes_256_but_not_257_per_camera():
    """256 masks pass the Python checks (the _NoGpu context then fails at the native call, not with ValueError); 257 do not."""
    ctx = _NoGpu()
    with pytest.raises(AttributeError):
        ctx.run_cams_wide([np.zeros((10, 4), np.float32)], [_cam(_u8(256)), _cam(_u8(0))])
    with pytest.raises(ValueError):
        ctx.run_cams_wide([np.zeros((10, 4), np.float32)], [_cam(_u8(256)), _cam(_u8(257))])


def _wide_frames(ids, counts, M=40):
    return [pipeline.FrameInputs(i, np.zeros((n, 4), np.float32), np.zeros((M, 48, 64), np.uint8), []) for i, n in zip(ids, counts)]


@pytest.mark.parametrize("frames_per_cam,ncams", [
    ([], 0),                                                                 # C = 0
    ([_wide_frames([1], [10])] * 5, 5),                                      # C = 5
    ([_wide_frames([1, 2], [10, 20]), _wide_frames([1, 3], [10, 20])], 2),   # frame ids differ
    ([_wide_frames([1, 2], [10, 20]), _wide_frames([1, 2], [10, 21])], 2),   # point counts differ
    ([_wide_frames([1, 2], [10, 20]), _wide_frames([1], [10])], 2),          # frame counts differ
    ([_wide_frames([1], [10], M=5), _wide_frames([1], [11], M=300)], 2),     # point counts differ, masks for every route
    ([_wide_frames([1], [10])], 2),                                          # frames for one camera, two cameras
])
def test_run_frames_multicam_with_wide_cameras_refuses_frames_that_differ(frames_per_cam, ncams):
    cams = [(np.eye(4), _Camera())] * ncams
    with pytest.raises(ValueError):
        pipeline.run_frames_multicam(frames_per_cam, cams, ctx=_NoGpu())
