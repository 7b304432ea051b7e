"""The multi-camera entry point (lpf_run_cams) without a GPU: the header declares it, the ctypes mirror of lpf_cam_input matches the C
layout (compiled and measured by gcc), and the Python entries refuse bad arguments before anything reaches the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lidar_object_detection_amd import _native, pipeline
from lidar_object_detection_amd._native import CamInput, LpfContext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lpf.h")


def test_header_declares_the_multicam_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+lpf_run_cams\s*\(", text)
    assert re.search(r"\}\s*lpf_cam_input\s*;", text)
    assert re.search(r"#define\s+LPF_MAX_CAMS\s+4\b", raw)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert "lpf_run_cams" in _native.EXPORTED
    assert _native.LPF_MAX_CAMS == 4


def test_cam_input_mirror_matches_the_header(tmp_path):
    names = [f[0] for f in CamInput._fields_]
    nested = ["masks.%s" % f[0] for f in _native.WideInput._fields_]
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%s %%zu\\n", "%s", offsetof(lpf_cam_input, %s));\n' % (f, f) for f in names + nested)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("sizeof %%zu\\n", sizeof(lpf_cam_input));\n'
                   '%s    return 0;\n}\n' % (HEADER, body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    lay = {k: int(v) for k, v in (line.split() for line in out if line)}
    assert lay["sizeof"] == ctypes.sizeof(CamInput) == 288
    for n in names:
        assert lay[n] == getattr(CamInput, n).offset, n
    for f in _native.WideInput._fields_:
        assert lay["masks." + f[0]] == CamInput.masks.offset + getattr(_native.WideInput, f[0]).offset, f[0]


class _NoGpu(LpfContext):
    """A context that never opened a device: any native call would fail with AttributeError, not ValueError."""
    def __init__(self):                      # (LpfContext.__init__ would create a GPU context)
        self.W, self.H = 64, 48
        self.box_off = None

    def __del__(self):
        pass


def _cam(masks=None, W=64, H=48, **kw):
    d = dict(T_velo_to_rect=np.eye(4), K=np.eye(3), width=W, height=H, masks=masks)
    d.update(kw)
    return d


@pytest.mark.parametrize("cams", [
    [],                                                                      # C = 0
    [_cam() for _ in range(5)],                                              # C = 5
    [_cam(np.zeros((33, 48, 64), np.uint8))],                                # M = 33: above LPF_MAX_MASKS per camera
    [_cam(), _cam(np.zeros((3, 48, 63), np.uint8))],                         # not camera 1's size
    [_cam(np.zeros((3, 40, 30), np.uint8), W=30, H=41)],                     # not this camera's size either
    [_cam(np.zeros((2, 3, 48, 64), np.uint8))],                              # two frames of masks for one frame of points
    [_cam(np.zeros((3, 48, 64), np.uint8), binarize="round")],
    [_cam(np.zeros((3, 48, 64), np.uint8), erode_iters=-1)],
    [_cam(np.zeros((3, 48, 64), np.uint8), rects=np.zeros((2, 4), np.int32))],
    [_cam(boxes=[np.zeros((1, 8, 3)), np.zeros((1, 8, 3))])],               # boxes for two frames
    [_cam(T_velo_to_rect=np.eye(3))],
])
def test_run_cams_refuses_bad_arguments_before_the_gpu(cams):
    ctx = _NoGpu()
    with pytest.raises(ValueError):
        ctx.run_cams([np.zeros((10, 4), np.float32)], cams)


class _Camera:
    def __init__(self, W=64, H=48):
        self.width, self.height, self.K = W, H, np.eye(3)


def _frames(ids, counts):
    return [pipeline.FrameInputs(i, np.zeros((n, 4), np.float32), [np.zeros((48, 64), np.uint8)], []) for i, n in zip(ids, counts)]


@pytest.mark.parametrize("frames_per_cam,ncams", [
    ([], 0),                                                                 # C = 0
    ([_frames([1], [10])] * 5, 5),                                           # C = 5
    ([_frames([1, 2], [10, 20]), _frames([1, 3], [10, 20])], 2),             # frame ids differ
    ([_frames([1, 2], [10, 20]), _frames([1, 2], [10, 21])], 2),             # point counts differ
    ([_frames([1, 2], [10, 20]), _frames([1], [10])], 2),                    # frame counts differ
    ([_frames([1], [10])], 2),                                               # frames for one camera, two cameras
])
def test_run_frames_multicam_refuses_frames_that_differ(frames_per_cam, ncams):
    cams = [(np.eye(4), _Camera())] * ncams
    with pytest.raises(ValueError):
        pipeline.run_frames_multicam(frames_per_cam, cams, ctx=_NoGpu())


def test_process_frames_multicam_refuses_bad_cameras():
    seg = lambda img: (None, [], [], [], [])                                 # noqa: E731
    for ids in [(), (0, 0), (0, 1, 2), (0, 1, 0, 1, 0)]:
        with pytest.raises(ValueError):
            pipeline.process_frames_multicam(cam_ids=ids, segmenter=seg, kitti360_path="/nonexistent")
