"""Per-car depth overlays (lpf_depth_overlays) without a GPU: the header declares the structs and the call, the ctypes mirrors match the
C layout, the committed jet table is matplotlib's and the kernels' table is the committed one, a NumPy restatement of
seg_with_pointcloud.py:174-180 reproduces every reference-generated golden hash, and the Python layer refuses bad inputs before a
context is made."""
import ctypes
import os
import re

import numpy as np
import pytest

import overlay_ref as R
from conftest import GOLDEN, load_calib
from lidar_object_detection_amd import _native, pipeline
from lidar_object_detection_amd._native import DepthOverlayInput, DepthOverlayOutputs
from oracle import cpu_oracle as orc
from test_wide_api import HEADER, _c_layout, _NoGpu

KERNELS = os.path.join(os.path.dirname(_native.__file__), "csrc", "lpf_depth_overlays.hip.h")


def test_header_declares_the_structs_and_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef\s+struct\s+lpf_depth_overlay_input\s*\{(.*?)\}\s*lpf_depth_overlay_input\s*;", text, flags=re.S)
    assert m, "lpf_depth_overlay_input is not declared"
    for f in ("pix", "car_off"):
        assert re.search(r"\bconst\s+int64_t\s*\*\s*%s\s*;" % f, m.group(1)), f
    assert re.search(r"\bconst\s+uint8_t\s*\*\s*seg\s*;", m.group(1))
    m = re.search(r"typedef\s+struct\s+lpf_depth_overlay_outputs\s*\{(.*?)\}\s*lpf_depth_overlay_outputs\s*;", text, flags=re.S)
    assert m and re.search(r"\buint8_t\s*\*\s*images\s*;", m.group(1)) and re.search(r"\bdouble\s*\*\s*max_depth\s*;", m.group(1))
    assert re.search(r"\bint\s+lpf_depth_overlays\s*\(\s*lpf_ctx\s*\*\s*ctx\s*,\s*int\s+F\s*,\s*const\s+lpf_depth_overlay_input\s*\*\s*in\s*,"
                     r"\s*const\s+lpf_depth_overlay_outputs\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert "lpf_depth_overlays" in _native.EXPORTED


@pytest.mark.parametrize("cls,struct,size", [(DepthOverlayInput, "lpf_depth_overlay_input", 56),
                                             (DepthOverlayOutputs, "lpf_depth_overlay_outputs", 24)])
def test_struct_mirrors_match_the_header(tmp_path, cls, struct, size):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls) == size
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n


def test_jet_table_ends():
    lut = R.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (0, 0, 127) and tuple(lut[-1]) == (127, 0, 0)


def test_jet_table_is_matplotlibs():
    pytest.importorskip("matplotlib")
    import matplotlib.pyplot as plt
    cm = plt.get_cmap("jet")
    x = np.arange(256) / 256.0                               # index i = min(255, int(256 * x)): i itself
    assert np.array_equal(np.uint8(cm(x)[..., :3] * 255), R.jet_lut())
    assert np.array_equal(np.uint8(cm(np.array([1.0]))[..., :3] * 255)[0], R.jet_lut()[255])     # x = 1 -> 256 -> 255


def test_kernel_table_is_the_committed_one():
    src = open(KERNELS).read()
    body = src[src.index("lpf_jet_u8[256][3] = {"):]
    body = body[:body.index("};")]
    vals = np.array([int(v) for v in re.findall(r"\d+", body.split("=", 1)[1])], np.int64)
    assert np.array_equal(vals.reshape(256, 3), R.jet_lut())


def _lists(pts, masks, cal):
    """the depth-map lists of a frame from the C oracle's last-writer image: flatnonzero(where(mask > 0.5, D, 0)) per car"""
    D, _ = orc.depth_image(pts, cal["TrVeloToRect"], np.asarray(cal["K"])[:3, :3], int(cal["width"]), int(cal["height"]), 0.0, R.DMAX)
    out = []
    for m in masks:
        p = np.flatnonzero(np.where(m > 0.5, D, 0.0))
        out.append((p, D.ravel()[p]))
    return out


def test_restatement_reproduces_every_golden_hash():
    cal = load_calib()
    H, W = int(cal["height"]), int(cal["width"])
    gold = R.load_overlay_golden()
    assert gold["H"] == H and gold["W"] == W and len(gold["frames"]) == 23
    inputs = R.golden_inputs(H, W)
    lut = R.jet_lut()
    g100 = np.load(os.path.join(GOLDEN, "frame_0000000100.npz"))
    n_cars = n_skipped = 0
    for rec in gold["frames"]:
        d = inputs[rec["key"]]
        assert rec["seg_seed"] == R.SEG_SEED + d["frame"] + (R.FULL_SEED_OFFSET if d["full"] else 0)
        for kind in ("rect5", "edge"):
            lists = _lists(d["pts"], d[kind], cal)
            assert len(lists) == len(rec[kind])
            if rec["key"] == "100" and kind == "rect5":         # the reference's own lists
                off = g100["depthmap_off_rect5"]
                for m, (p, dep) in enumerate(lists):
                    assert np.array_equal(p, g100["depthmap_idx_rect5"][off[m]:off[m + 1]])
                    assert np.array_equal(dep.view(np.int64), g100["depthmap_val_rect5"][off[m]:off[m + 1]].view(np.int64))
            for (p, dep), car in zip(lists, rec[kind]):
                img, mx = R.overlay(d["seg"], p, dep, lut)
                assert float.fromhex(car["max_hex"]) == mx and car["n_pixels"] == len(p), (rec["key"], kind, car["car_id"])
                assert car["skipped"] == (len(p) == 0)
                if car["skipped"]:
                    n_skipped += 1
                else:
                    assert R.sha(img) == car["sha256"], (rec["key"], kind, car["car_id"])
                    n_cars += 1
    assert n_cars > 150 and n_skipped > 10


# ---- the Python layer refuses bad inputs before any native call ------------------------------------------------------------------
def _car(pix, dep):
    return (np.asarray(pix, np.int64), np.asarray(dep, np.float64), None)


GOOD = [_car([1, 5], [2.0, 3.0]), _car([], [])]
SEG = np.zeros((1, 48, 64, 3), np.uint8)


@pytest.mark.parametrize("maps,seg,msg", [
    ([GOOD], np.zeros((1, 48, 63, 3), np.uint8), "camera's size"),
    ([GOOD], np.zeros((1, 48, 64), np.uint8), "camera's size"),
    ([GOOD], np.zeros((2, 48, 64, 3), np.uint8), "camera's size"),                      # two images for one frame
    ([GOOD], np.zeros((1, 48, 64, 3), np.float32), "uint8"),
    ([GOOD, GOOD[:1]], np.zeros((2, 48, 64, 3), np.uint8), "same number of cars"),       # ragged
    ([[_car([5, 1], [2.0, 3.0])]], SEG, "ascending"),
    ([[_car([1, 1], [2.0, 3.0])]], SEG, "ascending"),                                   # (strictly)
    ([[_car([-1, 3], [2.0, 3.0])]], SEG, "inside the image"),
    ([[_car([1, 64 * 48], [2.0, 3.0])]], SEG, "inside the image"),
    ([[_car([1, 2], [0.0, 3.0])]], SEG, "finite and > 0"),
    ([[_car([1, 2], [np.nan, 3.0])]], SEG, "finite and > 0"),
    ([[_car([1, 2], [np.inf, 3.0])]], SEG, "finite and > 0"),
    ([[_car([1, 2], [3.0])]], SEG, "same length"),
    ([[(np.array([1.0, 2.0]), np.array([1.0, 2.0]), None)]], SEG, "integer"),
    ([[_car([], [])] * 257], SEG, "at most 256"),
])
def test_depth_overlays_refuses_bad_inputs_before_the_gpu(maps, seg, msg):
    with pytest.raises(ValueError, match=msg):
        _NoGpu().depth_overlays(maps, seg)


class _Cam:
    width, height = 64, 48
    K = np.eye(3)


class _NoContext:
    def __getattr__(self, name):                            # any use of the context is a failure: the checks must come first
        raise AssertionError("the context was used: " + name)


@pytest.mark.parametrize("segs", [
    [np.zeros((48, 63, 3), np.uint8)],                                                  # off-size
    [np.zeros((48, 64), np.uint8)],                                                     # grey
    [np.zeros((48, 64, 4), np.uint8)],                                                  # RGBA
    [np.zeros((48, 64, 3), np.float64)],                                                # the script's / 255. image
    [np.zeros((48, 64, 3), np.uint8)] * 2,                                              # one image too many
    [],                                                                                 # one too few
])
def test_depth_overlays_frames_refuses_bad_segmented_images(segs):
    f = pipeline.FrameInputs(0, np.zeros((10, 4), np.float32), np.zeros((2, 48, 64), np.uint8))
    with pytest.raises(ValueError):
        pipeline.depth_overlays_frames([f], segs, np.eye(4), _Cam(), ctx=_NoContext())


def test_process_frames_depth_overlays_checks_its_arguments():
    with pytest.raises(ValueError, match="segment"):
        next(pipeline.process_frames_depth_overlays(0, 0, segmenter=None, kitti360_path="/nonexistent"))
    with pytest.raises(ValueError, match="cam_id"):
        next(pipeline.process_frames_depth_overlays(0, 2, segmenter=lambda im: None, kitti360_path="/nonexistent"))


def test_overlay_rows_pack_the_lists():
    pix, dep, off, M = _native.LpfContext.overlay_rows([[_car([3, 9], [1.5, 2.5]), _car([], []), _car([0], [4.0])],
                                                        [_car([], []), _car([7], [8.0]), _car([], [])]], 64 * 48)
    assert M == 3 and pix.shape == dep.shape == (2, 3)
    assert off.tolist() == [[0, 2, 2, 3], [0, 0, 1, 1]]
    assert pix[0].tolist() == [3, 9, 0] and pix[1, 0] == 7 and dep[0].tolist() == [1.5, 2.5, 4.0] and dep[1, 0] == 8.0
    pix, dep, off, M = _native.LpfContext.overlay_rows([], 10)
    assert M == 0 and pix.shape == (0, 0) and off.shape == (0, 1)
