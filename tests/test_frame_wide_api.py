"""The one-frame wide entry point (lpf_run_frame_wide) without a GPU: the header declares the job and the call, the library's export
list names it, the ctypes mirror matches the C layout (compiled and measured by gcc), and make_frame_step_wide refuses bad inputs
before anything reaches the native library."""
import ctypes
import re

import numpy as np
import pytest
import torch

from lidar_object_detection_amd import _native
from lidar_object_detection_amd._native import FrameJobWide, LpfContext, WideOutputs
from test_wide_api import HEADER, _c_layout, _NoGpu


def test_header_declares_the_job_and_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef\s+struct\s+lpf_frame_job_wide\s*\{(.*?)\}\s*lpf_frame_job_wide\s*;", text, flags=re.S)
    assert m, "lpf_frame_job_wide is not declared"
    assert re.search(r"\blpf_wide_outputs\s+out\s*;", m.group(1))
    assert re.search(r"\bint\s+lpf_run_frame_wide\s*\(\s*lpf_ctx\s*\*\s*ctx\s*,\s*const\s+lpf_frame_job_wide\s*\*\s*job\s*\)\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert "lpf_run_frame_wide" in _native.EXPORTED
    assert hasattr(LpfContext, "make_frame_step_wide")


def test_frame_job_wide_mirror_matches_the_header(tmp_path):
    names = [f[0] for f in FrameJobWide._fields_]
    lay = _c_layout(tmp_path, "lpf_frame_job_wide", names)
    assert lay["sizeof"] == ctypes.sizeof(FrameJobWide)
    for n in names:
        assert lay[n] == getattr(FrameJobWide, n).offset, n
    assert FrameJobWide.out.offset + ctypes.sizeof(WideOutputs) == ctypes.sizeof(FrameJobWide)


def test_stats_name_the_direct_frames_last():
    assert LpfContext.STATS[-1] == "wide_direct_frames"
    assert len(LpfContext.STATS) == 8


def _pts(n=10):
    return torch.zeros((n, 4), dtype=torch.float32)


def _m(M, H=48, W=64, dtype=None):
    return torch.zeros((M, H, W), dtype=dtype or torch.uint8)


@pytest.mark.parametrize("args,kw,msg", [
    ((_pts(), _m(257)), {}, "at most 256"),                                                     # M = 257: above LPF_MAX_MASKS_WIDE
    ((_pts(), _m(40, dtype=torch.float32)), {}, "masks_u8"),                                     # not uint8
    ((_pts(), _m(40, dtype=torch.bool)), {}, "masks_u8"),
    ((_pts(), torch.zeros((40, 48 * 64), dtype=torch.uint8)), {}, "masks_u8"),                   # not [M, H, W]
    ((_pts(), torch.zeros((1, 40, 48, 64), dtype=torch.uint8)), {}, "masks_u8"),
    ((_pts(), _m(40, W=63)), {}, "camera's size"),
    ((_pts(), np.zeros((40, 48, 64), np.uint8)), {}, "masks_u8"),                                # a NumPy array, not a tensor
    ((_pts(), _m(40)), {"mask_rects": torch.zeros((39, 4), dtype=torch.int32)}, "mask_rects"),   # one rectangle short
    ((_pts(), _m(40)), {"mask_rects": torch.zeros((40, 4), dtype=torch.int64)}, "mask_rects"),   # not int32
    ((_pts(), _m(40)), {"mask_rects": torch.zeros((4, 40), dtype=torch.int32).t()}, "mask_rects"),   # not contiguous
    ((_pts(), _m(40)), {"mask_rects": np.zeros((40, 4), np.int32)}, "mask_rects"),
    ((torch.zeros((10, 3)), _m(40)), {}, "pts"),
    ((torch.zeros((10, 4), dtype=torch.float64), _m(40)), {}, "pts"),
    ((_pts(), _m(40)), {"boxes_cam0": torch.zeros((3, 8, 3), dtype=torch.float32), "T_cam_to_velo": np.eye(4)}, "boxes_cam0"),
    ((_pts(), _m(40)), {"boxes_cam0": torch.zeros((3, 8, 3), dtype=torch.float64), "T_cam_to_velo": np.eye(3)}, "T_cam_to_velo"),
    ((_pts(), _m(40)), {"bogus": torch.zeros(3)}, "unknown"),
    ((_pts(), _m(40)), {}, "GPU tensor"),                                                       # host tensors
    ((_pts(), _m(0)), {"label_words": torch.zeros((10, 1), dtype=torch.int32)}, "GPU tensor"),
])
def test_make_frame_step_wide_refuses_bad_inputs_before_the_gpu(args, kw, msg):
    ctx = _NoGpu()
    with pytest.raises(ValueError, match=msg):
        ctx.make_frame_step_wide(*args, **kw)
