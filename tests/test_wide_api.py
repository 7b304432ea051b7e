"""The wide entry point (lpf_run_wide) without a GPU: the header declares it, the ctypes mirrors match the C layout of its two
structs (compiled and measured by gcc), and the Python entry refuses bad shapes before anything reaches the GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lidar_object_detection_amd import _native
from lidar_object_detection_amd._native import LpfContext, WideInput, WideOutputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "lpf.h")


def _header_text():
    return open(HEADER).read()


def test_header_declares_the_wide_call():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert re.search(r"\bint\s+lpf_run_wide\s*\(", text)
    assert "lpf_run_wide" in _native.EXPORTED
    assert re.search(r"#define\s+LPF_MAX_MASKS_WIDE\s+256\b", _header_text())
    assert re.search(r"#define\s+LPF_MAX_MASKS\s+32\b", _header_text())            # the narrow limit is unchanged
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", _header_text())
    assert _native.LPF_MAX_MASKS_WIDE == 256


def _c_layout(tmp_path, struct, fields):
    src = tmp_path / "layout.c"
    body = "".join('    printf("%%s %%zu\\n", "%s", offsetof(%s, %s));\n' % (f, struct, f) for f in fields)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n    printf("sizeof %%zu\\n", sizeof(%s));\n%s'
                   '    return 0;\n}\n' % (HEADER, struct, body))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    return {k: int(v) for k, v in (line.split() for line in out if line)}


@pytest.mark.parametrize("cls,struct", [(WideInput, "lpf_wide_input"), (WideOutputs, "lpf_wide_outputs")])
def test_struct_mirrors_match_the_header(cls, struct, tmp_path):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls)
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n
    assert ctypes.sizeof(WideInput) == 40 and ctypes.sizeof(WideOutputs) == 152


class _NoGpu(LpfContext):
    """A context that never opened a device: any native call would fail with AttributeError, not ValueError."""
    def __init__(self):                      # (LpfContext.__init__ would create a GPU context)
        self.W, self.H = 64, 48
        self.box_off = None

    def __del__(self):
        pass


@pytest.mark.parametrize("masks,kw,frames", [
    (np.zeros((257, 48, 64), np.uint8), {}, 1),                       # M = 257: above LPF_MAX_MASKS_WIDE
    (np.zeros((40, 48, 63), np.uint8), {}, 1),                        # not the camera's size
    (np.zeros((2, 40, 48, 64), np.uint8), {}, 1),                     # two frames of masks for one frame of points
    (np.zeros((40, 48, 64), np.uint8), {"binarize": "round"}, 1),
    (np.zeros((40, 48, 64), np.uint8), {"erode_iters": -1}, 1),
    (np.zeros((40, 48, 64), np.uint8), {"rects": np.zeros((39, 4), np.int32)}, 1),
    (np.zeros((40, 48, 64), "U1"), {}, 1),
])
def test_wide_entry_refuses_bad_shapes_before_the_gpu(masks, kw, frames):
    ctx = _NoGpu()
    pts = [np.zeros((10, 4), np.float32)] * frames
    with pytest.raises(ValueError):
        ctx.run_wide(pts, masks, **kw)


def test_wide_mask_batch_accepts_up_to_256():
    b = _native.wide_mask_batch(np.zeros((256, 4, 5), bool), 1, 4, 5, rects=np.zeros((256, 4), np.int32))
    m, M, is_f, dev, rects = b.masks, b.M, b.is_float, b.on_device, b.rects
    assert m.shape == (1, 256, 4, 5) and m.dtype == np.uint8 and M == 256 and not is_f and not dev and rects.shape == (1, 256, 4)
    assert b.form == "dense" and b.struct is None and b.tables is None and b.gpu is None
    assert b._fields[:5] == ("masks", "M", "is_float", "on_device", "rects")
    b = _native.wide_mask_batch(np.zeros((2, 33, 4, 5), np.float64), 2, 4, 5, binarize="gt0.5")
    assert b.masks.dtype == np.float32 and b.M == 33 and b.is_float is True and b.form == "dense"
