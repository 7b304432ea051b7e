"""Per-box point counts and point-level recall (lpf_box_points) without a GPU: the header declares the structs and the call, the ctypes
mirrors match the C layout, the library exports the symbol, the Python layer refuses bad inputs before any native call, and the NumPy
restatement (tests/box_points_ref.py) reproduces, bit for bit, the per-box sums and the first boxes the reference's own
oriented_point_in_bbox / point_in_bbox made on the committed frames (tests/golden/make_golden_box_points.py) -- every frame, both depth
windows, both box kinds, the frame without a box file and the one without a visible box included.  The GPU's outputs are held against
the same restatement in tests/test_gpu_box_points.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import box_points_ref as R
from conftest import GOLDEN, check_full, golden_frames, load_calib, load_golden, load_golden_full
from lidar_object_detection_amd import _build, _native, pipeline
from lidar_object_detection_amd._native import BoxPointsInput, BoxPointsOutputs
from test_wide_api import HEADER, _c_layout, _NoGpu

FULL = (1461, 2098, 2449)


def test_header_declares_the_structs_and_the_call():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"typedef\s+struct\s+lpf_box_points_input\s*\{(.*?)\}\s*lpf_box_points_input\s*;", text, flags=re.S)
    assert m, "lpf_box_points_input is not declared"
    for f in ("valid_idx", "n_valid"):
        assert re.search(r"\bconst\s+int64_t\s*\*\s*%s\s*;" % f, m.group(1)), f
    assert re.search(r"\bconst\s+uint32_t\s*\*\s*label_valid_words\s*;", m.group(1)) and re.search(r"\bint32_t\s+LW\s*;", m.group(1))
    m = re.search(r"typedef\s+struct\s+lpf_box_points_outputs\s*\{(.*?)\}\s*lpf_box_points_outputs\s*;", text, flags=re.S)
    assert m, "lpf_box_points_outputs is not declared"
    for f in ("box_points", "box_labelled", "first_box"):
        assert re.search(r"\bint32_t\s*\*\s*%s\s*;" % f, m.group(1)), f
    assert re.search(r"\bint64_t\s*\*\s*frame_counts\s*;", m.group(1))
    assert re.search(r"\bint\s+lpf_box_points\s*\(\s*lpf_ctx\s*\*\s*ctx\s*,\s*const\s+float\s*\*\s*pts\s*,\s*const\s+int64_t\s*\*\s*frame_off\s*,"
                     r"\s*int\s+F\s*,\s*int\s+pts_on_device\s*,\s*const\s+lpf_box_points_input\s*\*\s*in\s*,"
                     r"\s*const\s+lpf_box_points_outputs\s*\*\s*out\s*\)\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", raw)
    assert "lpf_box_points" in _native.EXPORTED
    assert "lpf_box_points.hip.h" in _build.SOURCES            # the build id covers the kernel's file


@pytest.mark.parametrize("cls,struct,size", [(BoxPointsInput, "lpf_box_points_input", 32), (BoxPointsOutputs, "lpf_box_points_outputs", 40)])
def test_struct_mirrors_match_the_header(tmp_path, cls, struct, size):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls) == size
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_exports_the_symbol():
    syms = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT lpf_box_points\b", syms)
    assert "lpf_box_points_kernel" in syms                     # the kernel is in the library's symbol table too


# ---- the Python layer refuses bad inputs before any native call ------------------------------------------------------------------
PTS = [np.zeros((10, 4), np.float32)]
VI, NV = np.arange(10, dtype=np.int64), np.array([4], np.int64)


def _ctx_with_boxes(F=1, B=3):
    c = _NoGpu()
    c.box_off = np.arange(F + 1, dtype=np.int32) * B
    return c


@pytest.mark.parametrize("args,kw,msg", [
    ((VI, NV), {"want": ("box_points", "recall")}, "want is a selection"),
    ((VI, NV), {"want": ()}, "want is a selection"),
    ((VI[:9], NV), {}, r"valid_idx \[Ntot\] and n_valid \[F\]"),
    ((VI.reshape(5, 2), NV), {}, r"valid_idx \[Ntot\] and n_valid \[F\]"),
    ((VI, np.array([4, 4], np.int64)), {}, r"valid_idx \[Ntot\] and n_valid \[F\]"),             # two frames of lists, one of points
    ((VI, NV.reshape(1, 1)), {}, r"valid_idx \[Ntot\] and n_valid \[F\]"),
    ((VI, NV, np.zeros(9, np.uint32)), {}, r"label_valid \[Ntot\] or \[Ntot, LW\]"),
    ((VI, NV, np.zeros((10, 9), np.uint32)), {}, r"label_valid \[Ntot\] or \[Ntot, LW\]"),
    ((VI, NV, np.zeros((10, 0), np.uint32)), {}, r"label_valid \[Ntot\] or \[Ntot, LW\]"),
    ((VI, NV, np.zeros((10, 2, 1), np.uint32)), {}, r"label_valid \[Ntot\] or \[Ntot, LW\]"),
    ((VI, NV), {"out": {"box_points": np.zeros(4, np.int32)}}, r"out\['box_points'\]"),
    ((VI, NV), {"out": {"first_box": np.zeros(10, np.int64)}}, r"out\['first_box'\]"),
    ((VI, NV), {"out": {"frame_counts": np.zeros((1, 3), np.int64)}}, r"out\['frame_counts'\]"),
])
def test_box_points_refuses_bad_inputs_before_the_gpu(args, kw, msg):
    with pytest.raises(ValueError, match=msg):
        _ctx_with_boxes().box_points(PTS, *args, **kw)


def test_box_points_refuses_missing_boxes_other_frames_and_mixed_memory():
    with pytest.raises(ValueError, match="boxes in force for no frames"):
        _NoGpu().box_points(PTS, VI, NV)
    with pytest.raises(ValueError, match="boxes in force for 2 frames, points of 1"):
        _ctx_with_boxes(F=2).box_points(PTS, VI, NV)
    with pytest.raises(ValueError, match=r"valid_idx \[Ntot\] and n_valid \[F\] of 3 points in 2 frames"):
        _ctx_with_boxes().box_points(None, VI, NV, staged=(np.array([0, 1, 3], np.int64), None, 0, None))

    class FakeGpuTensor:                                    # what _is_torch looks at: a type from a torch module, on the GPU
        is_cuda = True
        shape, dtype = (10,), "torch.int64"
    FakeGpuTensor.__module__ = "torch"
    with pytest.raises(ValueError, match="mixed"):
        _ctx_with_boxes().box_points(PTS, FakeGpuTensor(), NV)


def test_box_points_batch_describes_the_lists():
    assert _native.LpfContext.box_points_batch(VI, NV, None, 10, 1) == (False, 0)
    assert _native.LpfContext.box_points_batch(VI, NV, np.zeros(10, np.uint32), 10, 1) == (False, 1)
    assert _native.LpfContext.box_points_batch(VI, NV, np.zeros((10, 8), np.uint32), 10, 1) == (False, 8)


def test_point_recall_frames_refuses_before_the_gpu():
    assert pipeline.point_recall_frames([], None, None) == []
    for k in (2, 0, 17, 3.0, True):
        with pytest.raises(ValueError, match="erosion_kernel_size"):
            pipeline.point_recall_frames([object()], None, None, erosion_kernel_size=k)


# ---- the restatement reproduces the reference's own sums and first boxes, every frame ------------------------------------------------
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "box_points_golden.npz")))


def _cases():
    """(name, golden frame dict, is it a full-size one) of the 20 committed frames and the three full-size ones"""
    for rec in golden_frames()["frames"]:
        yield "%d" % rec["frame"], load_golden(rec["frame"]), False
    for frame in FULL:
        yield "%d_full" % frame, load_golden_full(frame), True


def test_restatement_reproduces_the_reference_sums_and_first_boxes_bit_for_bit():
    G = _golden()
    cal = load_calib()
    T, K3, W, H = cal["TrVeloToRect"], cal["K"][:3, :3], int(cal["width"]), int(cal["height"])
    assert G["frames"].tolist() == [r["frame"] for r in golden_frames()["frames"]] and len(G["frames"]) == 20
    assert G["full_frames"].tolist() == list(FULL)
    tot = dict(valid=0, boxes=0, empty=0, boxed=0, two=0, largest=0)
    seen = 0
    for name, g, full in _cases():
        pts = g["points"]
        corners = g["corners_velo"] if "corners_velo" in g else np.zeros((0, 8, 3))
        for win, dmax in R.WINDOWS:
            vi = R.valid_indices(pts, T, K3, W, H, dmax)       # the restated clip is the reference's: its indices, or their digest
            if full:
                check_full(g, "valid_idx_" + win, vi, np.int64)
            elif ("valid_idx_" + win) in g:
                assert np.array_equal(vi, g["valid_idx_" + win]), (name, win)
            for kind, oriented in R.KINDS:
                key = "%s_%s_%s_" % (name, win, kind)
                lab = np.zeros(len(vi), bool)
                lab[::3] = True
                r = R.frame_box_points(pts, vi, corners, lab, oriented)
                assert r["box_points"].dtype == np.int32 and np.array_equal(r["box_points"], G[key + "box_sum"]), key
                assert r["first_box"].dtype == np.int32 and np.array_equal(r["first_box"], G[key + "first"].astype(np.int32)), key
                per_point = r["inside"].sum(axis=0)
                assert int((per_point >= 2).sum()) == int(G[key + "two"]), key
                fc = r["frame_counts"]
                assert fc[0] == len(vi) and fc[1] == (r["first_box"] >= 0).sum() and fc[2] == lab.sum(), key
                assert fc[3] == (lab & (r["first_box"] >= 0)).sum() and np.all(r["box_labelled"] <= r["box_points"]), key
                assert r["box_points"].sum() >= fc[1] and (r["box_points"].sum() == fc[1]) == (int(G[key + "two"]) == 0), key
                c = R.confusion(fc)
                assert c["tp"] + c["fp"] + c["fn"] + c["tn"] == len(vi) and min(c.values()) >= 0, key
                seen += 1
                if not full and win == "d50" and oriented and len(corners):
                    tot["valid"] += len(vi); tot["boxes"] += len(corners); tot["empty"] += int((r["box_points"] == 0).sum())
                    tot["boxed"] += int(fc[1]); tot["two"] += int((per_point >= 2).sum())
                    tot["largest"] = max(tot["largest"], int(r["box_points"].max()))
    assert seen == 23 * 4
    # what the 18 sub-sampled frames with visible boxes hold (oriented, d50): the committed data exercises empty boxes and shared points
    assert tot == dict(valid=53843, boxes=472, empty=304, boxed=7077, two=681, largest=2945), tot


def test_restatement_counts_the_committed_masks():
    """rect5 masks on the committed frames (oriented, d50): labelled points in and out of boxes, count_mb below box_labelled"""
    tp = fp = fn = 0
    import inside_ref as IR
    for rec in golden_frames()["frames"]:
        g = load_golden(rec["frame"])
        if "corners_velo" not in g or not len(g["corners_velo"]):
            continue
        pts, lists, corners = IR.golden_frame_case(g, "rect5_d50")
        vi = g["valid_idx_d50"]
        r = R.recall_frame(pts, vi, lists, corners, pipeline.default_colors(len(lists)), 10, True)
        c = r["point_confusion"]
        tp += c["tp"]; fp += c["fp"]; fn += c["fn"]
        assert np.all(g["count_mb_rect5_d50"] <= r["box_labelled"][None, :]) and np.all(r["box_labelled"] <= r["box_points"])
        for d in r["car_statistics"]:
            if d["matched_bbox_id"] >= 0:
                assert d["bbox_lidar_points"] >= d["points_inside_bbox"] > 0
                assert d["recall_percentage"] == d["points_inside_bbox"] / d["bbox_lidar_points"] * 100
            else:
                assert d["bbox_lidar_points"] == 0 and d["recall_percentage"] == 0.0
    assert (tp, fp, fn) == (4744, 3367, 2333)


# ---- host-side pieces of the pipeline ------------------------------------------------------------------------------------------------
def test_recall_rows_columns():
    stats = [{"car_id": 0, "matched_bbox_id": 3, "total_points": 40, "points_inside_bbox": 30, "points_outside_bbox": 10,
              "inside_percentage": 75.0, "outside_percentage": 25.0, "color": (0, 0, 0), "bbox_lidar_points": 90,
              "recall_percentage": 30 / 90 * 100},
             {"car_id": 2, "matched_bbox_id": -1, "total_points": 5, "points_inside_bbox": 0, "points_outside_bbox": 5,
              "inside_percentage": 0.0, "outside_percentage": 100.0, "color": (1, 1, 1), "bbox_lidar_points": 0, "recall_percentage": 0.0}]
    rows = pipeline.recall_rows([dict(frame=7, car_statistics=stats), dict(frame=8, car_statistics=[])], timestamp="t")
    assert pipeline.RECALL_COLUMNS == pipeline.CSV_COLUMNS + ("bbox_lidar_points", "recall_percentage")
    assert len(rows) == 2 and all(tuple(r.keys()) == pipeline.RECALL_COLUMNS for r in rows)
    assert rows[0]["frame"] == 7 and rows[0]["bbox_lidar_points"] == 90 and rows[0]["recall_percentage"] == 33.33 and rows[0]["is_matched"]
    assert rows[1]["bbox_lidar_points"] == 0 and rows[1]["recall_percentage"] == 0.0 and not rows[1]["is_matched"]
    base = pipeline.csv_rows(stats, 7, "t")                    # csv_rows itself is unchanged: the rows' first columns are its rows
    assert tuple(base[0].keys()) == pipeline.CSV_COLUMNS and all(rows[0][k] == base[0][k] for k in pipeline.CSV_COLUMNS)
