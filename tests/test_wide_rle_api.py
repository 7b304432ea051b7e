"""Run-length masks in the wide and multi-camera passes, without a GPU: the header names the forms of lpf_wide_input.f32 (LPF_MASKS_RLE
= 2) with the ABI and the struct layouts unchanged, the library carries the wide decode kernel, every refusal of run_wide / run_cams /
run_cams_wide / run_frames_multicam is a ValueError raised before any native call, and rle_batch pads ragged frames up to the pass's
limit (against the independent NumPy restatement of tests/rle_ref.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rle_ref as R
from lidar_object_detection_amd import _build, _native, pipeline
from lidar_object_detection_amd._native import CamInput, RleMasksInput, WideInput
from lidar_object_detection_amd.rle import RleMasks
from test_wide_api import _NoGpu, _c_layout, _header_text


def test_header_names_the_forms_and_keeps_the_abi(tmp_path):
    text = _header_text()
    for name, value in (("LPF_MASKS_U8", 0), ("LPF_MASKS_F32", 1), ("LPF_MASKS_RLE", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", text)
    assert (_native.LPF_MASKS_U8, _native.LPF_MASKS_F32, _native.LPF_MASKS_RLE) == (0, 1, 2)
    # no layout change: sizes and offsets as they were (lpf_wide_input 40 bytes, lpf_cam_input 288)
    names = [f[0] for f in WideInput._fields_]
    lay = _c_layout(tmp_path, "lpf_wide_input", names)
    assert lay["sizeof"] == ctypes.sizeof(WideInput) == 40
    assert [lay[n] for n in names] == [getattr(WideInput, n).offset for n in names] == [0, 8, 16, 20, 24, 28, 32, 36]
    names = [f[0] for f in CamInput._fields_]
    lay = _c_layout(tmp_path, "lpf_cam_input", names)
    assert lay["sizeof"] == ctypes.sizeof(CamInput) == 288
    assert [lay[n] for n in names] == [getattr(CamInput, n).offset for n in names] == [0, 128, 200, 204, 208, 216, 224, 264, 272, 280, 284]
    assert ctypes.sizeof(RleMasksInput) == 32
    # the "not taken" paragraph no longer lists the three passes
    para = text[text.index("Not taken in this form"):text.index("typedef struct lpf_rle_masks")]
    assert "lpf_depth_maps" in para and "lpf_run_frame_wide" in para and "lpf_run_cams" not in para and "lpf_run_wide," not in para


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_carries_the_wide_decode_kernel():
    syms = subprocess.run(["nm", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"lpf_rle_decode_wide", syms)
    for lt in ("IhE", "ItE", "IjE"):                         # the narrow decode's three instantiations are still there
        assert re.search(r"lpf_rle_decode%s" % lt, syms), lt


def _rle(M, H=48, W=64, seed=0):
    return RleMasks.from_dense((np.random.default_rng(seed).random((M, H, W)) < 0.1).astype(np.uint8))


def test_rle_batch_with_the_wide_limit():
    a, b, c = _rle(40, seed=1), _rle(0), _rle(256, seed=2)
    runs, off, F, M = _native.LpfContext.rle_batch([a, b, c], 48, 64, 256, "run_wide")
    assert (F, M) == (3, 256) and runs.dtype == np.int32 and off.dtype == np.int64 and off.shape == (3 * 256 + 1,)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(runs) == len(a.runs) + len(c.runs)
    # frame 0: its 40 masks, then 216 empty ones; frame 1: 256 empty ones; frame 2: all its own
    assert np.array_equal(off[:41], a.run_off) and (off[40:513] == len(a.runs)).all()
    assert np.array_equal(off[512:], len(a.runs) + c.run_off)
    for f, (r, m) in enumerate(((a, 40), (b, 0), (c, 256))):
        dense = R.masks_to_dense(runs, off[f * M:(f + 1) * M + 1], M, 48, 64)
        assert np.array_equal(dense[:m], r.to_dense()) and not dense[m:].any(), f
    # the narrow limit and its messages are the default, as before
    with pytest.raises(ValueError, match=r"^set_masks_rle: frame 1 has 33 masks, one pass takes 32 \(pipeline.run_frames groups them\)$"):
        _native.LpfContext.rle_batch([a[:3], _rle(33)], 48, 64)
    with pytest.raises(ValueError, match=r"^run_wide: frame 0 has 257 masks, one pass takes 256"):
        _native.LpfContext.rle_batch(_rle(257), 48, 64, 256, "run_wide")
    with pytest.raises(ValueError, match=r"^set_masks_rle: frame 0 has masks of 63 x 48, the camera is 64 x 48 \(runs are not resized\)$"):
        _native.LpfContext.rle_batch(_rle(2, W=63), 48, 64)


def test_compact_mask_batch_builds_the_struct():
    a, b = _rle(40, seed=3), _rle(33, seed=4)
    batch = _native.compact_mask_batch([a, b], 2, 48, 64, erode_iters=2, forms=("rle",))
    (runs, off), inp, M = batch.tables, batch.struct, batch.M
    assert (M, batch.form, batch.on_device, batch.rects) == (40, "rle", False, None)
    assert batch.is_float is False and batch.masks is None and batch.gpu is None
    assert (inp.F, inp.M, inp.erode_iters, inp.reserved) == (2, 40, 2, 0)
    assert inp.runs == runs.ctypes.data and inp.run_off == off.ctypes.data
    ctx = _NoGpu()
    wi = WideInput()
    ctx._wide_input(wi, batch, "astype", 2)
    assert (wi.masks, wi.rects, wi.M, wi.f32, wi.binarize, wi.erode_iters, wi.on_device) == (ctypes.addressof(inp), None, 40, 2, 0, 2, 0)
    # arrays are not the form: the dense path's business
    assert _native.compact_mask_batch(np.zeros((40, 48, 64), np.uint8), 1, 48, 64, forms=("rle",)) is None
    assert _native.compact_mask_batch([np.zeros((40, 48, 64), np.uint8)], 1, 48, 64, forms=("rle",)) is None


_PTS = [np.zeros((10, 4), np.float32)]


def _cam(masks, **kw):
    return dict(T_velo_to_rect=np.eye(4), K=np.eye(3), width=64, height=48, masks=masks, **kw)


@pytest.mark.parametrize("what", ["mixed list", "mixed list, array first", "wrong size", "rects", "binarize", "v3_pipeline", "257 masks",
                                  "two frames for one", "erode_iters", "spoiled runs"])
def test_run_wide_refuses_before_the_gpu(what):
    ctx = _NoGpu()                                           # 64 x 48; any native call would be an AttributeError
    good = _rle(40)
    dense = np.zeros((40, 48, 64), np.uint8)
    frames, kw = _PTS, {}
    if what == "mixed list":
        frames, masks = _PTS * 2, [good, dense]
    elif what == "mixed list, array first":
        frames, masks = _PTS * 2, [dense, good]
    elif what == "wrong size":
        masks = _rle(40, W=63)
    elif what == "rects":
        masks, kw = good, dict(rects=np.zeros((1, 40, 4), np.int32))
    elif what == "binarize":
        masks, kw = good, dict(binarize="gt0.5")
    elif what == "v3_pipeline":
        masks, kw = good, dict(v3_pipeline=True)
    elif what == "257 masks":
        masks = _rle(257)
    elif what == "two frames for one":
        masks = [good, good]
    elif what == "erode_iters":
        masks, kw = good, dict(erode_iters=-1)
    else:
        masks = _rle(40)
        masks.runs = np.array([[64 * 48 - 2, 3]], np.int32)
        masks.run_off = np.array([0] + [1] * 40, np.int64)
    with pytest.raises(ValueError):
        ctx.run_wide(frames, masks, **kw)


@pytest.mark.parametrize("entry,limit", [("run_cams", 32), ("run_cams_wide", 256)])
@pytest.mark.parametrize("what", ["mixed list", "wrong size", "rects", "binarize", "v3_pipeline", "too many", "second camera"])
def test_camera_passes_refuse_before_the_gpu(entry, limit, what):
    ctx = _NoGpu()
    good = _rle(5)
    dense = np.zeros((5, 48, 64), np.uint8)
    frames = _PTS
    cams = {"mixed list": lambda: [_cam([good, dense])],
            "wrong size": lambda: [_cam(_rle(5, H=24, W=32))],        # (another camera's size: runs are not resized)
            "rects": lambda: [_cam(good, rects=np.zeros((1, 5, 4), np.int32))],
            "binarize": lambda: [_cam(good, binarize="v3")],
            "v3_pipeline": lambda: [_cam(good, v3_pipeline=True)],
            "too many": lambda: [_cam(_rle(limit + 1))],
            "second camera": lambda: [_cam(good), _cam(_rle(5, W=63))]}[what]()
    if what == "mixed list":
        frames = _PTS * 2
    with pytest.raises(ValueError) as e:
        getattr(ctx, entry)(frames, cams)
    if what == "second camera":
        assert str(e.value).startswith("%s: camera 1: " % entry)
    if what == "too many":
        assert "%d masks" % (limit + 1) in str(e.value) and "takes %d" % limit in str(e.value)


class _Cam:
    width, height = 64, 48
    K = np.eye(3)


@pytest.mark.parametrize("what", ["mixed", "wrong size"])
def test_run_frames_multicam_refuses_before_the_gpu(what):
    pts = np.zeros((10, 4), np.float32)
    dense = np.zeros((2, 48, 64), np.uint8)
    cam1 = {"mixed": [pipeline.FrameInputs(1, pts, _rle(2)), pipeline.FrameInputs(2, pts, dense)],
            "wrong size": [pipeline.FrameInputs(1, pts, _rle(2, H=24, W=32)), pipeline.FrameInputs(2, pts, None)]}[what]
    cam0 = [pipeline.FrameInputs(1, pts, _rle(2)), pipeline.FrameInputs(2, pts, _rle(3))]

    class _Ctx(_NoGpu):                                      # (the erosion element is set before the cameras are looked at)
        def set_erosion_element(self, k):
            pass

    with pytest.raises(ValueError):
        pipeline.run_frames_multicam([cam0, cam1], [(np.eye(4), _Cam()), (np.eye(4), _Cam())], ctx=_Ctx())
