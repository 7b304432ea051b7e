"""The batched box-view filter and box projection (lpf_box_views) without a GPU: the header declares the structs and the call, the
ctypes mirrors match the C layout, the library exports the symbol and the kernel, the Python layer refuses bad inputs before any native
call, the NumPy restatement (tests/box_views_ref.py) equals the scalar functions of the package and the three golden sets made by the
reference's own functions (tests/golden/make_golden_box_views.py) bit for bit, and the three batched pipeline functions equal the
scalar ones in lists, stats and printed lines on a context whose box_views is the restatement (the GPU's is held against the same
restatement in tests/test_gpu_box_views.py)."""
import contextlib
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

import box_views_ref as R
from conftest import GOLDEN, load_calib
from lidar_object_detection_amd import _build, _native, kitti360, pipeline
from lidar_object_detection_amd._native import BoxViewsInput, BoxViewsOutputs
from test_wide_api import HEADER, _c_layout, _NoGpu


def test_header_declares_the_structs_and_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef\s+struct\s+lpf_box_views_input\s*\{(.*?)\}\s*lpf_box_views_input\s*;", text, flags=re.S)
    assert m, "lpf_box_views_input is not declared"
    for f in ("corners_cam0", "T_cam_to_velo"):
        assert re.search(r"\bconst\s+double\s*\*\s*%s\s*;" % f, m.group(1)), f
    assert re.search(r"\bconst\s+int32_t\s*\*\s*box_off\s*;", m.group(1))
    assert re.search(r"\bint32_t\s+min_points_in_view\s*;", m.group(1)) and re.search(r"\bdouble\s+depth_lo\s*,\s*depth_hi\s*;", m.group(1))
    assert re.search(r"\bdouble\s+min_area\s*;", m.group(1))
    m = re.search(r"typedef\s+struct\s+lpf_box_views_outputs\s*\{(.*?)\}\s*lpf_box_views_outputs\s*;", text, flags=re.S)
    assert m, "lpf_box_views_outputs is not declared"
    assert re.search(r"\buint8_t\s*\*\s*keep\s*;", m.group(1))
    for f in ("reason", "corners_in_view", "corners_near", "front", "kept_pos", "frame_counts"):
        assert re.search(r"\bint32_t\s*\*\s*%s\s*;" % f, m.group(1)), f
    for f in ("avg_depth", "near_bbox2d", "bbox2d", "front_avg_depth", "corners_velo"):
        assert re.search(r"\bdouble\s*\*\s*%s\s*;" % f, m.group(1)), f
    assert re.search(r"\bint\s+lpf_box_views\s*\(\s*lpf_ctx\s*\*\s*ctx\s*,\s*int\s+F\s*,\s*const\s+lpf_box_views_input\s*\*\s*in\s*,"
                     r"\s*const\s+lpf_box_views_outputs\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert "lpf_box_views" in _native.EXPORTED
    assert [f[0] for f in BoxViewsOutputs._fields_[:12]] == list(_native.LpfContext.BOX_VIEWS_WANT) == list(R.WANT)
    assert _native.LpfContext.BOX_VIEW_REASONS == R.REASONS == pipeline._VIEW_REASONS


@pytest.mark.parametrize("cls,struct,size", [(BoxViewsInput, "lpf_box_views_input", 56), (BoxViewsOutputs, "lpf_box_views_outputs", 104)])
def test_struct_mirrors_match_the_header(tmp_path, cls, struct, size):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls) == size
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_exports_the_symbol_and_the_kernel():
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT lpf_box_views\b", syms)
    assert "lpf_box_views_kernel" in syms                    # the kernel is in the library's symbol table too


# ---- the Python layer refuses bad inputs before any native call ------------------------------------------------------------------
C5 = np.zeros((5, 8, 3), np.float64)
OFF = np.array([0, 2, 5])


@pytest.mark.parametrize("corners,box_off,kw,msg", [
    (np.zeros((5, 8, 2)), OFF, {}, r"\[Btot,8,3\]"),
    (np.zeros((5, 7, 3)), OFF, {}, r"\[Btot,8,3\]"),
    (np.zeros((40, 3)), OFF, {}, r"\[Btot,8,3\]"),
    (np.zeros((5, 8, 3), "U1"), OFF, {}, "must be numbers"),
    (C5, np.array([0, 2, 4]), {}, "rise from 0 to the 5 boxes"),
    (C5, np.array([1, 2, 5]), {}, "rise from 0 to the 5 boxes"),
    (C5, np.array([0, 3, 2, 5]), {}, "without a decrease"),
    (C5, np.array([[0, 5]]), {}, r"integers \[F\+1\]"),
    (C5, np.array([0.0, 5.0]), {}, r"integers \[F\+1\]"),
    (C5, np.zeros(0, np.int64), {}, r"integers \[F\+1\]"),
    (C5, OFF, {"want": ("keep", "depths")}, "want is a selection"),
    (C5, OFF, {"want": ()}, "want is a selection"),
    (C5, OFF, {"want": ("corners_velo",)}, "needs T_cam_to_velo"),
    (C5, OFF, {"want": ("corners_velo",), "T_cam_to_velo": np.eye(3)}, "4 x 4"),
    (C5, OFF, {"depth_range": (0.1, float("inf"))}, "finite"),
    (C5, OFF, {"depth_range": (float("nan"), 100)}, "finite"),
    (C5, OFF, {"depth_range": (0.1,)}, r"depth_range is \(lo, hi\)"),
    (C5, OFF, {"min_area": float("nan")}, "finite"),
    (C5, OFF, {"min_points_in_view": 9}, r"0\.\.8"),
    (C5, OFF, {"min_points_in_view": -1}, r"0\.\.8"),
    (C5, OFF, {"min_points_in_view": 2.5}, r"0\.\.8"),
])
def test_box_views_refuses_bad_inputs_before_the_gpu(corners, box_off, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _NoGpu().box_views(corners, box_off, **kw)


def test_box_views_refuses_gpu_corners_of_another_dtype():
    class FakeGpuTensor:                                    # what _is_torch looks at: a type from a torch module, on the GPU
        is_cuda = True
        shape, dtype = (5, 8, 3), "torch.float32"
    FakeGpuTensor.__module__ = "torch"
    with pytest.raises(ValueError, match="GPU corners must be float64"):
        _NoGpu().box_views(FakeGpuTensor(), OFF)


def test_box_views_batch_describes_the_call():
    dev, off, want = _native.LpfContext.box_views_batch(C5.astype(np.float32), [0, 0, 5, 5], want=["kept_pos", "frame_counts"])
    assert not dev and off.dtype == np.int32 and off.tolist() == [0, 0, 5, 5] and want == ("kept_pos", "frame_counts")
    dev, off, _ = _native.LpfContext.box_views_batch(np.zeros((0, 8, 3)), [0])
    assert not dev and off.tolist() == [0]


# ---- the restatement equals the goldens (the reference's own functions) and the scalar functions of the package ------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "box_views_golden.npz"))


def golden_set(z, name):
    return {k[2:]: z[k] for k in z.files if k.startswith(name + "_")}


def camera_of(z, name):
    cal = load_calib()
    if name == "c":
        K = np.eye(4)
        K[:3, :3] = z["c_K"]
        return kitti360.CameraPerspective.from_arrays(K, cal["R_rect"], int(z["c_size"][0]), int(z["c_size"][1]))
    return kitti360.CameraPerspective.from_arrays(cal["K"], cal["R_rect"], int(cal["width"]), int(cal["height"]))


def dicts_of(o):
    off = o["box_off"]
    return [[{"index": i, "corners_cam0": c.tolist()} for i, c in enumerate(o["corners"][a:b])] for a, b in zip(off[:-1], off[1:])]


@pytest.mark.parametrize("name,boxes,frames", [("a", 992, 19), ("b", 1500, 12), ("c", 116, 1)])
def test_restatement_reproduces_the_goldens(golden, name, boxes, frames):
    o = golden_set(golden, name)
    cam = camera_of(golden, name)
    assert len(o["corners"]) == boxes and len(o["box_off"]) == frames + 1
    got = R.views(o["corners"], o["box_off"], cam.K, cam.width, cam.height, np.eye(4))
    R.compare_with_fields(got, o, name)
    assert np.array_equal(got["frame_counts"][:, 0], o["kept_count"])
    reasons = str(o["filter_reasons"]).split("\n")
    for f, line in enumerate(reasons):                      # the counts per reason of the reference's stats
        exp = np.zeros(6, np.int64)
        for why, n in eval(line).items():
            exp[R.REASONS.index(why)] = n
        assert np.array_equal(got["frame_counts"][f, 1:], exp[1:]), (name, f)
    off = o["box_off"]
    for f in range(frames):                                 # kept_pos: the rank among the frame's kept boxes
        k = got["keep"][off[f]:off[f + 1]].astype(bool)
        assert np.array_equal(got["kept_pos"][off[f]:off[f + 1]], np.where(k, np.cumsum(k) - 1, -1))
    counts = np.bincount(got["reason"], minlength=6)
    if name != "a":
        assert all(counts[r] > 0 for r in (0, 2, 3, 4))
        assert set(got["corners_near"].tolist()) == set(range(9)) == set(got["front"].tolist())
    if name == "b":
        assert np.array_equal(o["corners"], R.seeded_boxes(1500, 0)) and all(counts[r] >= 200 for r in (0, 2, 3, 4))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_restatement_equals_the_scalar_functions(golden, name):
    o = golden_set(golden, name)
    cam = camera_of(golden, name)
    step = 1 if name == "c" else 3                           # (every third box of the larger sets: the scalar functions take 80 us a box)
    corners = o["corners"][::step]
    boxes = [{"corners_cam0": c.tolist()} for c in corners]
    exp = R.scalar_fields(boxes, cam, pipeline.is_bbox_in_camera_view, pipeline.project_3d_bbox_to_2d)
    for k, v in exp.items():                                 # the package's scalar functions give what the reference's gave
        assert R.same_bits(v, o[k][::step]), (name, k)
    Tcv = np.linalg.inv(load_calib()["TrVeloToCam"])
    got = R.views(corners, [0, len(corners)], cam.K, cam.width, cam.height, Tcv)
    R.compare_with_fields(got, exp, name)
    done = pipeline.transform_bboxes_to_velodyne([dict(b) for b in boxes], load_calib()["TrVeloToCam"])
    assert R.same_bits(got["corners_velo"], np.array([b["corners_velo"] for b in done]).reshape(-1, 8, 3))
    # other thresholds: against the scalar function with the same arguments
    kw = dict(min_points_in_view=6, depth_range=(2.0, 60.0))
    got = R.views(corners, [0, len(corners)], cam.K, cam.width, cam.height, None, min_area=100, want=("keep", "reason", "avg_depth"), **kw)
    for i, b in enumerate(boxes):
        ok, info = pipeline.is_bbox_in_camera_view(b, cam, **kw)
        assert ok == bool(got["keep"][i]) and info["reason"] == R.REASONS[got["reason"][i]], (name, i)
        if ok:
            assert info["avg_depth"] == got["avg_depth"][i]


def test_mean_is_in_numpy_order():
    rng = np.random.default_rng(5)
    d = rng.uniform(0.1, 100.0, (4000, 8)) * 10.0 ** rng.integers(-3, 4, (4000, 8))
    m = rng.random((4000, 8)) < 0.8
    m[:500] = True
    got = R.mean_in_numpy_order(d, m)
    exp = np.array([np.mean(d[i][m[i]]) if m[i].any() else 0.0 for i in range(len(d))])
    assert R.same_bits(got, exp)
    plain = np.array([sum(d[i][m[i]].tolist()) / max(int(m[i].sum()), 1) for i in range(len(d))])
    assert (plain[:500] != exp[:500]).any()                  # (eight values left to right are another number: the check can tell)


# ---- the batched pipeline functions equal the scalar ones: lists, stats and printed lines ---------------------------------------------
def _frames_for_pipeline(golden):
    o = golden_set(golden, "a")
    frames = dicts_of(o)
    frames[1][3] = {"index": 3}                                              # no corners
    frames[2][0] = {"index": 0, "corners_cam0": o["corners"][0][:4].tolist()}   # four corners: the scalar function's business
    frames[2][5] = {"index": 5, "corners_cam0": "none"}                        # an error
    return frames + [[], None, [{"index": 0}]], camera_of(golden, "a")


def _quiet(fn, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        r = fn(*a, **k)
    return r, buf.getvalue()


@pytest.mark.parametrize("verbose", [True, False])
def test_batched_filter_equals_the_scalar_one(golden, verbose):
    frames, cam = _frames_for_pipeline(golden)
    ctx = R.RefContext(cam.K, cam.width, cam.height)
    got, text = _quiet(pipeline.filter_bboxes_in_camera_view_frames, frames, cam, verbose=verbose, ctx=ctx)
    assert ctx.calls == {"box_views": 1, "match_2d": 0}
    exp_text = ""
    for f, boxes in enumerate(frames):
        (kept, stats), t = _quiet(pipeline.filter_bboxes_in_camera_view, boxes, cam, verbose)
        exp_text += t
        assert len(got[f][0]) == len(kept) and all(a is b for a, b in zip(got[f][0], kept)), f       # the same dict objects
        assert repr(got[f][1]) == repr(stats) and list(got[f][1]["filter_reasons"]) == list(stats["filter_reasons"]), f
    assert text == exp_text
    if verbose:
        z = golden_set(golden, "a")
        for needle in ("Depths: min=", "2D bbox: [np.int64(", "Projected area:", "no_corners", "[ERROR] Error checking bbox visibility"):
            assert needle in text, needle
        ref = str(z["stdout"])                               # the reference's own printed lines, on the frame left as it is
        assert text.startswith(ref[:ref.index("Filter reasons")])
    else:
        assert "[INFO]" not in text


def test_batched_filter_prints_the_references_lines(golden):
    for name in ("a", "b", "c"):
        o = golden_set(golden, name)
        cam = camera_of(golden, name)
        ctx = R.RefContext(cam.K, cam.width, cam.height)
        got, text = _quiet(pipeline.filter_bboxes_in_camera_view_frames, dicts_of(o), cam, ctx=ctx)
        assert text == str(o["stdout"]), name
        assert [s["kept"] for _, s in got] == o["kept_count"].tolist()
        assert "\n".join(repr(s["filter_reasons"]) for _, s in got) == str(o["filter_reasons"])


@pytest.mark.parametrize("detailed", [True, False])
def test_batched_projection_equals_the_scalar_one(golden, detailed):
    frames, cam = _frames_for_pipeline(golden)
    frames = frames[:4] + frames[-3:]
    ctx = R.RefContext(cam.K, cam.width, cam.height)
    got, text = _quiet(pipeline.project_3d_bboxes_to_2d_frames, frames, cam, detailed, ctx=ctx)
    assert ctx.calls["box_views"] == 1
    exp_text, n_none = "", 0
    for f, boxes in enumerate(frames):
        assert len(got[f]) == len(boxes or [])
        for j, b in enumerate(boxes or []):
            (info, corners), t = _quiet(pipeline.project_3d_bbox_to_2d, b, cam, detailed)
            exp_text += t
            gi, gc = got[f][j]
            assert repr(gi) == repr(info), (f, j)                        # the same values of the same types
            n_none += info is None
            if info is not None:
                assert type(gc) is np.ndarray and gc.dtype == corners.dtype and np.array_equal(gc, corners)
            else:
                assert gc is None
    assert text == exp_text and "[ERROR] Failed to project 3D bbox" in text and n_none > 20


def test_batched_secondtest_match_equals_the_scalar_composition(golden):
    cal = load_calib()
    z = np.load(os.path.join(GOLDEN, "match2d_golden.npz"))
    o = golden_set(golden, "a")
    assert z["frames"].tolist() == golden["a_frames"].tolist()
    base = dicts_of(o)
    cam = camera_of(golden, "a")
    dets = [z["%d_dets" % f] for f in z["frames"].tolist()] + [np.zeros((0, 4), np.float32), z["%d_dets" % z["frames"][0]], z["%d_dets" % z["frames"][1]]]
    colors = [pipeline.generate_consistent_colors(max(len(d) - 1, 0)) for d in dets]

    def fresh():
        frames = [[dict(b) for b in fr] for fr in base] + [[dict(b) for b in base[0]], [], [dict(b) for b in base[1]]]
        frames[1][3] = {"index": 3}
        frames[2][0] = {"index": 0, "corners_cam0": o["corners"][o["box_off"][2] + 1][:4].tolist()}
        return frames

    ours, theirs = fresh(), fresh()
    ctx = R.RefContext(cam.K, cam.width, cam.height)
    got, text = _quiet(pipeline.secondtest_match_frames, dets, ours, colors, cam, cal["TrVeloToCam"], ctx=ctx)
    assert ctx.calls == {"box_views": 1, "match_2d": 1}
    exp_text, n_matched = "", 0
    for f in range(len(dets)):
        def scalar():
            kept, stats = pipeline.filter_bboxes_in_camera_view(theirs[f], cam)
            boxes = pipeline.transform_bboxes_to_velodyne(kept, cal["TrVeloToCam"])
            return pipeline.improved_match_detections_to_bboxes(dets[f], boxes, colors[f], cam), stats, boxes
        (matched, stats, boxes), t = _quiet(scalar)
        exp_text += t
        gm, gs, gb = got[f]
        assert repr(gs) == repr(stats) and len(gm) == len(matched) and len(gb) == len(boxes), f
        assert all(a is b for a, b in zip(gb, [b for b in ours[f] if any(b is k for k in gb)])), f       # the caller's own dicts
        for (gc, gcol), (ec, ecol) in zip(gm, matched):
            assert type(gc) is type(ec) and gc.dtype == ec.dtype and np.array_equal(gc, ec), f
            assert type(gcol) is type(ecol) and np.array_equal(np.asarray(gcol), np.asarray(ecol)), f
        n_matched += sum(1 for _, col in matched if not isinstance(col, list))
        assert repr(ours[f]) == repr(theirs[f]), f               # the callers' dicts changed as the composition changes them: no more
    assert text == exp_text
    assert n_matched > 20 and "[INFO] Matched detection" in text and "[STATS] BBox Filtering Results:" in text
    assert "[INFO] No detections or 3D bounding boxes to match" in text
