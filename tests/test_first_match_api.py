"""Same_color's first-mask labels for a batch (lpf_first_match) without a GPU: the header declares the structs and the call, the ctypes
mirrors match the C layout, the library exports the symbol and the kernels, the Python layer refuses bad inputs before any native
call, and the NumPy restatement (tests/first_match_ref.py) reproduces, bit for bit, what the script's own lines Same_color.py:114-132
made of the committed frames and of the constructed cases (tests/golden/make_golden_first_match.py).  The constructed cases are
regenerated here from their seeds, and what they have to reach is asserted.  The GPU's outputs are held against the same restatement
in tests/test_gpu_first_match.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import first_match_ref as R
from conftest import GOLDEN, golden_frames, load_calib, load_golden
from lidar_object_detection_amd import _build, _native, pipeline
from lidar_object_detection_amd._native import FirstMatchInput, FirstMatchOutputs
from test_wide_api import HEADER, _c_layout, _NoGpu


def test_header_declares_the_structs_and_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef\s+struct\s+lpf_first_match_input\s*\{(.*?)\}\s*lpf_first_match_input\s*;", text, flags=re.S)
    assert m, "lpf_first_match_input is not declared"
    assert re.search(r"\bconst\s+void\s*\*\s*masks\s*;", m.group(1)) and re.search(r"\bconst\s+double\s*\*\s*colors\s*;", m.group(1))
    for f in ("M", "mh, mw", "f32", "on_device", "reserved"):
        assert re.search(r"\bint32_t\s+%s\s*;" % f, m.group(1)), f
    m = re.search(r"typedef\s+struct\s+lpf_first_match_outputs\s*\{(.*?)\}\s*lpf_first_match_outputs\s*;", text, flags=re.S)
    assert m, "lpf_first_match_outputs is not declared"
    for f, t in (("first_mask", "int32_t"), ("car_idx", "int64_t"), ("car_mask", "int32_t"), ("car_xyz", "float"), ("car_rgb", "double"),
                 ("bg_idx", "int64_t"), ("bg_xyz", "float"), ("mask_count", "int64_t")):
        assert re.search(r"\b%s\s*\*\s*%s\s*;" % (t, f), m.group(1)), f
    assert re.search(r"\bint64_t\s*\*\s*n_valid\s*,\s*\*\s*n_car\s*,\s*\*\s*n_bg\s*;", m.group(1))
    assert re.search(r"\bint\s+lpf_first_match\s*\(\s*lpf_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*pts\s*,\s*const\s+int64_t\s*\*\s*frame_off\s*,"
                     r"\s*int\s+F\s*,\s*int\s+pts_on_device\s*,\s*const\s+lpf_first_match_input\s*\*\s*in\s*,"
                     r"\s*const\s+lpf_first_match_outputs\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert re.search(r"8 \(continued\): lpf_first_match_input, lpf_first_match_outputs, lpf_first_match \(added; nothing else\s+changed\)", raw)
    assert "lpf_first_match" in _native.EXPORTED
    assert "lpf_first_match.hip.h" in _build.SOURCES           # the build id covers the kernels' file


@pytest.mark.parametrize("cls,struct,size", [(FirstMatchInput, "lpf_first_match_input", 40), (FirstMatchOutputs, "lpf_first_match_outputs", 96)])
def test_struct_mirrors_match_the_header(tmp_path, cls, struct, size):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls) == size
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_exports_the_symbol_and_the_kernels():
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT lpf_first_match\b", syms)
    for k in ("lpf_fm_count", "lpf_fm_scan", "lpf_fm_scatter"):
        assert k in syms, k                                     # the kernels are in the library's symbol table too


# ---- the Python layer refuses bad inputs before any native call ------------------------------------------------------------------
PTS = [np.zeros((10, 4), np.float32)]
MASKS = np.zeros((1, 3, 20, 30), np.uint8)
COLORS = np.zeros((1, 3, 3), np.float64)


class FakeGpuTensor:                                        # what _is_torch looks at: a type from a torch module, on the GPU
    is_cuda = True
    shape, dtype = (1, 3, 20, 30), "torch.uint8"


FakeGpuTensor.__module__ = "torch"


@pytest.mark.parametrize("masks,kw,msg", [
    (MASKS, {"want": ("car_idx", "colours")}, "want is a selection"),
    (MASKS, {"want": ()}, "want is a selection"),
    (MASKS, {"want": ("car_rgb",)}, "car_rgb is wanted, colors is None"),
    (np.zeros((2, 3, 20, 30), np.uint8), {}, r"masks \[F,M,mh,mw\] for 1 frames"),                # two frames of masks, one of points
    (np.zeros((20, 30), np.uint8), {}, r"masks \[F,M,mh,mw\] for 1 frames"),
    (np.zeros((1, 257, 2, 2), np.uint8), {}, "257 masks per frame, one call takes 256"),
    (np.zeros((1, 3, 0, 30), np.uint8), {}, "masks of 0 x 30 pixels"),
    (np.zeros((1, 3, 20, 30), "U1"), {}, "masks must be uint8, bool or float"),
    (MASKS, {"colors": np.zeros((1, 2, 3))}, r"colors \[F,M,3\]"),
    (MASKS, {"colors": np.zeros((1, 3, 4))}, r"colors \[F,M,3\]"),
    (MASKS, {"colors": FakeGpuTensor()}, "mixed"),
    (MASKS, {"out": {"car_idx": np.zeros(9, np.int64)}}, r"out\['car_idx'\]"),
    (MASKS, {"out": {"first_mask": np.zeros(10, np.int64)}}, r"out\['first_mask'\]"),
    (MASKS, {"out": {"mask_count": np.zeros((1, 4), np.int64)}}, r"out\['mask_count'\]"),
])
def test_first_match_refuses_bad_inputs_before_the_gpu(masks, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _NoGpu().first_match(PTS, masks, **kw)


def test_first_match_batch_describes_the_masks():
    fmb = _native.LpfContext.first_match_batch
    dev, M, mh, mw, f32, m, c = fmb(MASKS, COLORS, 1)
    assert (dev, M, mh, mw, f32) == (False, 3, 20, 30, 0) and m.dtype == np.uint8 and c.dtype == np.float64
    dev, M, mh, mw, f32, m, c = fmb(np.zeros((4, 7, 9), np.float64), None, 1)            # one frame: [M,mh,mw]
    assert (dev, M, mh, mw, f32) == (False, 4, 7, 9, 1) and m.dtype == np.float32 and m.shape == (1, 4, 7, 9) and c is None
    assert fmb(np.zeros((2, 0, 1, 1), bool), None, 2)[:5] == (False, 0, 1, 1, 0)


def test_pipeline_refuses_before_the_gpu():
    assert pipeline.first_match_frames([], None, None) == []
    with pytest.raises(ValueError, match="one list of colours per frame"):
        pipeline.first_match_frames([pipeline.FrameInputs(0, PTS[0], [])], None, None, mask_colors=[[], []])
    with pytest.raises(ValueError, match="needs the segmentation callable"):
        next(pipeline.process_frames_same_color())

    class Cam:
        width, height = 30, 20
    fr = [pipeline.FrameInputs(0, PTS[0], [np.zeros((20, 30), np.float32), np.zeros((20, 30, 1), np.float32)])]
    with pytest.raises(ValueError, match=r"masks must be a list of \[h,w\] arrays"):
        pipeline.first_match_frames(fr, None, Cam())
    fr = [pipeline.FrameInputs(0, PTS[0], [np.zeros((20, 30), np.float32)] * 2, colors=[(1, 2, 3)])]
    with pytest.raises(ValueError, match="2 masks, 1 colours"):
        pipeline.first_match_frames(fr, None, Cam())


def test_masks_go_down_at_their_own_size_and_ragged_lists_on_the_canvas():
    class Cam:
        width, height = 30, 20
    same = [pipeline.FrameInputs(0, PTS[0], [np.ones((12, 40), np.float32)] * 2), pipeline.FrameInputs(1, PTS[0], np.ones((3, 12, 40), bool))]
    batch, Ms = pipeline._first_match_masks(same, Cam())
    assert batch.shape == (2, 3, 12, 40) and batch.dtype == np.float32 and Ms == [2, 3]      # one size: no canvas, padded with an empty plane
    assert batch[0, :2].all() and not batch[0, 2].any() and batch[1].all()
    ragged = [pipeline.FrameInputs(0, PTS[0], [np.ones((12, 40), np.uint8), np.full((25, 10), 7, np.uint8)]), pipeline.FrameInputs(1, PTS[0], [])]
    batch, Ms = pipeline._first_match_masks(ragged, Cam())
    assert batch.shape == (2, 2, 20, 30) and batch.dtype == np.uint8 and Ms == [2, 0]
    assert batch[0, 0, :12].all() and not batch[0, 0, 12:].any() and batch[0, 1, :, :10].all() and not batch[0, 1, :, 10:].any()
    none, Ms = pipeline._first_match_masks([pipeline.FrameInputs(0, PTS[0], None)], Cam())
    assert none.shape[:2] == (1, 0) and Ms == [0]


# ---- the restatement reproduces the script's own lines, bit for bit -------------------------------------------------------------------
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "first_match_golden.npz")))


def _projected(pts, cal):
    return R.project(pts, cal["TrVeloToRect"], cal["K"][:3, :3], int(cal["width"]), int(cal["height"]))


def _equals_golden(G, key, r):
    assert np.array_equal(r["car_idx"], G[key + "_car"]) and np.array_equal(r["car_mask"], G[key + "_mask"]), key
    assert np.array_equal(r["bg_idx"], G[key + "_bg"]), key
    assert r["mask_count"].sum() == len(r["car_idx"]) and r["first_mask"].dtype == np.int32, key


def test_restatement_equals_the_script_on_every_committed_frame():
    G, cal = _golden(), load_calib()
    frames = [rec["frame"] for rec in golden_frames()["frames"]]
    assert G["frames"].tolist() == frames and len(frames) == 20
    car = bg = 0
    for fr in frames:
        g = load_golden(fr)
        pts, masks = R.golden_frame_case(g, cal)
        u, v, valid = _projected(pts, cal)
        if "u" in g:
            assert np.array_equal(u, g["u"]) and np.array_equal(v, g["v"])           # the reference's own pixels
        if "valid_idx_d30" in g:
            assert np.array_equal(np.flatnonzero(valid), g["valid_idx_d30"])
        r = R.first_match(u, v, valid, masks, [(i, i, i) for i in range(len(masks))])
        _equals_golden(G, "f%d" % fr, r)
        assert np.array_equal(r["car_rgb"][:, 0] * 255.0, r["car_mask"].astype(np.float64))
        car += len(r["car_idx"]); bg += len(r["bg_idx"])
    assert (car, bg) == (29667, 23221)                      # (what the generator printed: the script's own totals)


def test_restatement_equals_the_script_on_the_constructed_cases_and_they_reach_what_they_must():
    G, cal = _golden(), load_calib()
    W, H = int(cal["width"]), int(cal["height"])
    assert G["cases"].tolist() == list(R.CASES)
    seen = {}
    for name in R.CASES:
        pts, masks = R.constructed_case(name, cal)
        u, v, valid = _projected(pts, cal)
        r = R.first_match(u, v, valid, masks)
        _equals_golden(G, name, r)
        seen[name] = (u, v, valid, masks, r)
    # a point in two or more masks whose first and last mask differ; a point whose only mask is the last one
    for name in ("overlap_f32", "overlap_u8"):
        u, v, valid, masks, r = seen[name]
        inside = np.array([[bool(valid[i]) and mk[v[i], u[i]] > 0.5 for i in range(len(u))] for mk in masks])
        many = inside.sum(axis=0) >= 2
        last = len(masks) - 1 - np.argmax(inside[::-1], axis=0)
        assert (many & (r["first_mask"] != last)).any(), name
        only_last = (inside.sum(axis=0) == 1) & inside[-1]
        assert only_last.any() and np.all(r["first_mask"][only_last] == len(masks) - 1), name
        assert masks[0].dtype == (np.float32 if name == "overlap_f32" else np.uint8)
    # masks smaller and larger than the image; valid points at u = mw-1, u = mw, v = mh-1 and v = mh of the smaller ones
    u, v, valid, masks, r = seen["small"]
    mh, mw = masks[0].shape
    assert mh < H and mw < W
    for at in ((u == mw - 1) & (v < mh), (u == mw) & (v < mh), (v == mh - 1) & (u < mw), (v == mh) & (u < mw)):
        assert (valid & at).any()
    assert np.all(r["first_mask"][valid & ((u >= mw) | (v >= mh))] == -1) and np.all(r["first_mask"][valid & (u < mw) & (v < mh)] >= 0)
    u, v, valid, masks, r = seen["large"]
    assert masks[0].shape == (H + 5, W + 7) and (valid & (u == W - 1) & (v == H - 1)).any() and np.all(r["first_mask"][valid] >= 0)
    # the float values around 0.5, each under a valid point that no earlier mask takes
    u, v, valid, masks, r = seen["values"]
    n = len(R.FLOAT_VALUES)
    assert valid[:n].all()
    got = masks[0][v[:n], u[:n]]
    assert got.tobytes() == np.array(R.FLOAT_VALUES, np.float32).tobytes()
    assert got[1] == np.float32(0.5) + np.float32(2.0 ** -24) and got[5] == np.float32(2.0 ** -149) and np.isnan(got[2])
    assert r["first_mask"][:n].tolist() == [0 if mem else 1 for mem in R.FLOAT_MEMBER]
    # a frame with no mask; a frame with no valid point
    u, v, valid, masks, r = seen["no_mask"]
    assert masks == [] and valid.any() and len(r["car_idx"]) == 0 and len(r["bg_idx"]) == valid.sum()
    u, v, valid, masks, r = seen["no_valid"]
    assert len(masks) == 2 and not valid.any() and np.all(r["first_mask"] == -2)


def test_golden_stores_indices_and_mask_ids_only():
    G = _golden()
    assert os.path.getsize(os.path.join(GOLDEN, "first_match_golden.npz")) < 256 * 1024
    for k, a in G.items():
        assert k in ("frames", "cases") or (k.rsplit("_", 1)[1] in ("car", "mask", "bg") and a.ndim == 1 and a.dtype.kind == "i"), k
