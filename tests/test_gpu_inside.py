"""lpf_inside_masks / LpfContext.inside_masks / car_statistics_v3_frames / inside_outside_cloud_frames on the GPU, against the NumPy
restatement of V3's inside / outside split (tests/inside_ref.py, pinned to the reference's own masks by tests/test_inside_api.py) --
never against the library's own lpf_points_in_boxes, except where the issue is that the batched dicts equal the per-frame ones.
Every committed frame takes part, the one without a box file and the one without a visible box included."""
import contextlib
import io
import os

import numpy as np
import pytest

import inside_ref as R
from conftest import golden_frames, load_golden, unpack_masks
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd._native import LpfContext
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp

pytestmark = pytest.mark.gpu
RECS = golden_frames()["frames"]                                 # all 20: frame 570 has no visible box, frame 2717 no box file
TAGS = ("rect5_d50", "rect5_d30", "edge_d50")
ROWS = ("inside", "part_idx", "part_xyz")


def _camera(calib):
    return kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))


@pytest.fixture(scope="module")
def cal(calib):
    _, T, K, W, H = S.default_calibration(calib)
    return dict(T=T, K=K, W=W, H=H, calib=calib)


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


def _golden_batch(cal, tag):
    """the committed frames under ``tag``: (points, masks uint8 [m,H,W], corners, reference lists) per frame"""
    kind, dmax = tag.split("_d")
    out = []
    for rec in RECS:
        g = load_golden(rec["frame"])
        masks = unpack_masks(g, kind, cal["H"], cal["W"]).astype(np.uint8) if ("masks_%s_packed" % kind) in g else np.zeros((0, cal["H"], cal["W"]), np.uint8)
        pts, lists, corners = R.golden_frame_case(g, tag)
        assert len(lists) == len(masks)
        out.append(dict(frame=rec["frame"], points=pts, masks=masks, corners=corners, lists=lists, g=g))
    return out, float(dmax)


def _narrow_pass(ctx, cal, frames, dmax, oriented, M=None):
    """set_camera / set_masks / set_boxes / run_batch over ``frames`` (masks padded to M with empty ones) -> (res, M)"""
    M = max(len(f["masks"]) for f in frames) if M is None else M
    stack = np.zeros((len(frames), M, cal["H"], cal["W"]), np.uint8)
    for i, f in enumerate(frames):
        stack[i, :len(f["masks"])] = f["masks"]
    ctx.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, dmax)
    ctx.set_masks(stack)
    ctx.set_boxes([f["corners"] for f in frames], oriented=oriented)
    return ctx.run_batch([f["points"] for f in frames], want_uv=False, want_label=False), M


def _check_frame(split, i, M, ref, why, count_mb=None):
    """frame i of inside_masks' arrays against frame_split's dict ``ref`` (m <= M real cars: the others are empty and unmatched)"""
    m = len(ref["matched"])
    tot = int(ref["off"][-1])
    assert np.array_equal(split["inside"][i, :tot], ref["inside"]), why
    assert np.array_equal(split["part_idx"][i, :tot], ref["part_idx"]), why
    assert np.array_equal(split["part_xyz"][i, :tot].view(np.uint32), ref["part_xyz"].view(np.uint32)), why
    assert np.array_equal(split["n_inside"][i, :m], ref["n_inside"]) and not split["n_inside"][i, m:].any(), why
    assert np.array_equal(split["matched"][i, :m], ref["matched"]) and not split["matched"][i, m:].any(), why
    assert not split["inside"][i, tot:].any() and not split["part_idx"][i, tot:].any() and not split["part_xyz"][i, tot:].any(), why
    for car in range(m):                                         # the bytes of a matched car sum to its count in its best box
        a, e = int(ref["off"][car]), int(ref["off"][car + 1])
        n = int(split["inside"][i, a:e].sum())
        assert n == int(split["n_inside"][i, car]), why + (car,)
        if ref["matched"][car]:
            assert n == int(ref["count_mb"][car, ref["best_box"][car]]) == int(ref["best_cnt"][car]), why + (car,)
            if count_mb is not None:
                assert n == int(count_mb[car, ref["best_box"][car]]), why + (car,)


@pytest.mark.parametrize("oriented", [True, False], ids=["oriented", "aabb"])
@pytest.mark.parametrize("tag", TAGS)
def test_golden_frames_every_car(ctx, cal, tag, oriented):
    frames, dmax = _golden_batch(cal, tag)
    refs = [R.frame_split(f["points"], f["lists"], f["corners"], 10, oriented) for f in frames]
    res, M = _narrow_pass(ctx, cal, frames, dmax, oriented)
    arrs = pipeline.inside_list_arrays(res, M)
    split = ctx.inside_masks([f["points"] for f in frames], *arrs, min_points=10)
    assert split["inside"].dtype == np.uint8 and split["part_idx"].dtype == np.int64 and split["part_xyz"].dtype == np.float32
    assert split["n_inside"].dtype == np.int64 and split["matched"].dtype == np.int32
    matched = 0
    for i, (f, r, ref) in enumerate(zip(frames, res, refs)):
        m = len(f["lists"])
        for a, b in zip(r["inst_lists"][:m], f["lists"]):        # the run's lists are the reference's
            assert np.array_equal(a, b)
        assert np.array_equal(r["best_box"][:m], ref["best_box"]) and np.array_equal(r["best_cnt"][:m], ref["best_cnt"])
        gold = f["g"].get(("count_mb_" if oriented else "count_mb_aabb_") + tag)
        if gold is not None:
            assert np.array_equal(r["count_mb"][:m], gold) and np.array_equal(ref["count_mb"], gold)
        _check_frame(split, i, M, ref, (tag, oriented, f["frame"]), r["count_mb"])
        matched += int(ref["matched"].sum())
    assert matched >= 30                                         # (124 over the three tags, oriented)
    # all frames in one batch equal each frame alone
    for i, f in enumerate(frames):
        one, M1 = _narrow_pass(ctx, cal, [f], dmax, oriented)
        s1 = ctx.inside_masks([f["points"]], *pipeline.inside_list_arrays(one, M1), min_points=10)
        tot = int(refs[i]["off"][-1])
        m = len(f["lists"])
        for k in ROWS:
            assert np.array_equal(s1[k][0, :tot], split[k][i, :tot]), (tag, f["frame"], k)
        for k in ("n_inside", "matched"):
            assert np.array_equal(s1[k][0, :m], split[k][i, :m]), (tag, f["frame"], k)


def test_host_and_device_io_and_null_outputs(ctx, cal):
    import torch
    frames, dmax = _golden_batch(cal, "edge_d50")
    res, M = _narrow_pass(ctx, cal, frames, dmax, True)
    arrs = pipeline.inside_list_arrays(res, M)
    pts = [f["points"] for f in frames]
    host = ctx.inside_masks(pts, *arrs)
    dev = torch.device("cuda", 0)
    tarrs = [torch.from_numpy(a).to(dev) for a in arrs]
    got = ctx.inside_masks(pts, *tarrs)
    torch.cuda.synchronize(dev)
    for k in LpfContext.INSIDE_WANT:
        assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy().view(np.uint8), host[k].view(np.uint8)), k
    # device points (one tensor per frame), host lists
    got = ctx.inside_masks([torch.from_numpy(p).to(dev) for p in pts], *arrs)
    for k in LpfContext.INSIDE_WANT:
        assert np.array_equal(got[k].view(np.uint8), host[k].view(np.uint8)), k
    # device lists, host outputs are not a combination of the Python entry; any selection of outputs gives the same arrays
    for want in (("inside",), ("part_idx",), ("part_xyz",), ("n_inside",), ("matched",), ("part_xyz", "matched"), ("inside", "n_inside")):
        for a, name in ((arrs, "host"), (tarrs, "device")):
            part = ctx.inside_masks(pts, *a, want=want)
            assert tuple(part) == want
            for k in want:
                v = part[k].cpu().numpy() if name == "device" else part[k]
                assert np.array_equal(v.view(np.uint8), host[k].view(np.uint8)), (want, name, k)
    # what the call does not write stays as it was: entries beyond a frame's lists, in host and in device memory
    tot = arrs[1][:, M]
    assert (tot < arrs[0].shape[1]).any()
    fill = dict(inside=np.full(host["inside"].shape, 9, np.uint8), part_idx=np.full(host["part_idx"].shape, -7, np.int64),
                part_xyz=np.full(host["part_xyz"].shape, 2.5, np.float32))
    for name in ("host", "device"):
        out = {k: (v.copy() if name == "host" else torch.from_numpy(v).to(dev)) for k, v in fill.items()}
        part = ctx.inside_masks(pts, *(arrs if name == "host" else tarrs), want=ROWS, out=out)
        for k in ROWS:
            v = part[k] if name == "host" else part[k].cpu().numpy()
            for i in range(len(frames)):
                assert np.array_equal(v[i, :tot[i]], host[k][i, :tot[i]]) and np.array_equal(v[i, tot[i]:], fill[k][i, tot[i]:]), (name, k, i)


def test_device_lists_with_host_outputs_through_the_c_abi(ctx, cal):
    """the one combination LpfContext.inside_masks does not offer: lists in device memory, outputs in host memory (the call reads the
    lists' offsets back first, to know how much of each row to return)"""
    import ctypes
    import torch
    from lidar_object_detection_amd._native import InsideInput, InsideOutputs
    frames, dmax = _golden_batch(cal, "rect5_d50")
    res, M = _narrow_pass(ctx, cal, frames, dmax, True)
    arrs = pipeline.inside_list_arrays(res, M)
    pts = [f["points"] for f in frames]
    host = ctx.inside_masks(pts, *arrs)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in arrs]
    torch.cuda.synchronize(dev)
    off, ptr, pdev, _keep = ctx.stage_points(pts)
    F, cap = arrs[0].shape
    inp, o = InsideInput(), InsideOutputs()
    inp.inst_idx, inp.inst_off, inp.best_box, inp.best_cnt = (x.data_ptr() for x in t)
    inp.inst_cap, inp.M, inp.min_points, inp.on_device = cap, M, 10, 1
    out = dict(inside=np.full((F, cap), 9, np.uint8), part_idx=np.full((F, cap), -7, np.int64), part_xyz=np.full((F, cap, 3), 2.5, np.float32),
               n_inside=np.full((F, M), -1, np.int64), matched=np.full((F, M), -1, np.int32))
    for k, v in out.items():
        setattr(o, k, v.ctypes.data)
    ctx._check(ctx._lib.lpf_inside_masks(ctx._h, ptr, off.ctypes.data, F, pdev, ctypes.byref(inp), ctypes.byref(o)))
    tot = arrs[1][:, M]
    for k in ("n_inside", "matched"):
        assert np.array_equal(out[k], host[k]), k
    for k in ROWS:
        for i in range(F):
            assert np.array_equal(out[k][i, :tot[i]], host[k][i, :tot[i]]), (k, i)
            assert (out[k][i, tot[i]:] == (9 if k == "inside" else -7 if k == "part_idx" else 2.5)).all(), (k, i)


def _wide_masks(M, seed, W, H):
    """M disk masks that overlap (the same disk several times), some of them empty"""
    m, _ = S.synthetic_disk_masks(M, seed, W, H)
    rng = np.random.default_rng(seed)
    for i in rng.choice(M, size=M // 7, replace=False):
        m[i] = 0
    m[M // 2] = m[1]
    m[M - 1] = m[1] | m[2]
    return m


def _ref_lists(cal, points, masks, dmax=50.0):
    """the reference's own statements (V3:565-592, V3:211-233): the instance lists of one frame"""
    return npp.frame_path(points, cal["T"], cal["K"], cal["W"], cal["H"], dmax, masks, np.zeros((0, 8, 3)))[3]


@pytest.mark.parametrize("M", [33, 64, 256])
def test_wide_path_equals_the_reference_and_the_mask_group_run(ctx, cal, M):
    g = load_golden(100)                                         # the full-size frame: 109 355 points, 25 visible boxes
    pts, corners = g["points"], g["corners_velo"]
    masks = _wide_masks(M, 40 + M, cal["W"], cal["H"])
    ctx.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, 50.0)
    ctx.set_boxes([corners], oriented=True)
    res = ctx.run_wide([pts], masks, want_uv=False)
    lists = _ref_lists(cal, pts, masks)
    for a, b in zip(res[0]["inst_lists"], lists):
        assert np.array_equal(a, b)
    ref = R.frame_split(pts, lists, corners, 10, True)
    assert ref["matched"].sum() >= 3 and (ref["matched"] == 0).sum() >= 3 and any(len(l) == 0 for l in lists)
    arrs = pipeline.inside_list_arrays(res, M)
    split = ctx.inside_masks([pts], *arrs, min_points=10)
    _check_frame(split, 0, M, ref, ("wide", M), res[0]["count_mb"])
    # the same frame once per group of 32 masks through the narrow path
    for g0 in range(0, M, 32):
        grp = dict(points=pts, masks=masks[g0:g0 + 32], corners=corners)
        r32, m32 = _narrow_pass(ctx, cal, [grp], 50.0, True)
        s32 = ctx.inside_masks([pts], *pipeline.inside_list_arrays(r32, m32), min_points=10)
        a, e = int(ref["off"][g0]), int(ref["off"][g0 + m32])
        for k in ROWS:
            assert np.array_equal(s32[k][0, :e - a], split[k][0, a:e]), (M, g0, k)
        assert np.array_equal(s32["n_inside"][0], split["n_inside"][0, g0:g0 + m32])
        assert np.array_equal(s32["matched"][0], split["matched"][0, g0:g0 + m32])


def test_a_frame_whose_lists_did_not_fit_is_left_alone(ctx, cal):
    g = load_golden(100)
    pts, corners = g["points"], g["corners_velo"]
    M = 40
    masks = _wide_masks(M, 7, cal["W"], cal["H"])
    few = masks.copy()
    few[8:] = 0                                                  # frame 0 lists less than frame 1
    ctx.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, 50.0)
    ctx.set_boxes([corners, corners], oriented=True)
    res = ctx.run_wide([pts, pts], np.stack([few, masks]), want_uv=False)
    idx, off, bb, bc = pipeline.inside_list_arrays(res, M)
    cap = int(off[0, M])
    assert 0 < cap < int(off[1, M])                              # with room for frame 0 only, frame 1 has overflowed
    ref0 = R.frame_split(pts, _ref_lists(cal, pts, few), corners, 10, True)
    ref1 = R.frame_split(pts, _ref_lists(cal, pts, masks), corners, 10, True)
    out = dict(inside=np.full((2, cap), 9, np.uint8), part_idx=np.full((2, cap), -7, np.int64), part_xyz=np.full((2, cap, 3), 2.5, np.float32))
    split = ctx.inside_masks([pts, pts], np.ascontiguousarray(idx[:, :cap]), off, bb, bc, min_points=10, out=out)
    assert np.array_equal(split["inside"][0], ref0["inside"]) and np.array_equal(split["part_idx"][0], ref0["part_idx"])
    assert np.array_equal(split["part_xyz"][0], ref0["part_xyz"]) and np.array_equal(split["n_inside"][0], ref0["n_inside"])
    assert (split["inside"][1] == 9).all() and (split["part_idx"][1] == -7).all() and (split["part_xyz"][1] == 2.5).all()
    assert not split["n_inside"][1].any() and np.array_equal(split["matched"][1], ref1["matched"]) and ref1["matched"].any()


# ---- the statistics dicts and the cloud ----------------------------------------------------------------------------------------------
def _same_dicts(got, want, why):
    assert len(got) == len(want), why
    for a, b in zip(got, want):
        assert list(a.keys()) == list(b.keys()), why
        for k in a:
            x, y = a[k], b[k]
            if isinstance(y, np.ndarray):
                assert isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), why + (k,)
            else:
                assert type(x) is type(y) and x == y, why + (k, x, y)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _boxes(corners):
    return [{"corners_cam0": None, "corners_velo": c.tolist()} for c in corners]


def _items(cal, tag):
    frames, dmax = _golden_batch(cal, tag)
    return [pipeline.FrameInputs(f["frame"], f["points"], f["masks"], _boxes(f["corners"]), pipeline.default_colors(len(f["masks"])))
            for f in frames], frames, dmax


@pytest.mark.parametrize("tag", ["rect5_d50", "edge_d50", "rect5_d30"])
@pytest.mark.parametrize("oriented", [True, False], ids=["oriented", "aabb"])
def test_statistics_dicts_equal_the_per_frame_ones_and_the_reference(cal, tag, oriented):
    items, frames, dmax = _items(cal, tag)
    cam = _camera(cal["calib"])
    T = cal["calib"]["TrVeloToRect"]
    got = pipeline.car_statistics_v3_frames(items, T, cam, dmax, 10, oriented)
    base = pipeline.run_frames(items, T, cam, dmax, 10, oriented)
    n = 0
    for r, b, it, f in zip(got, base, items, frames):
        why = (tag, oriented, f["frame"])
        per_frame = _quiet(pipeline.calculate_car_point_statistics, b["car_point_sets"], it.bboxes_3d, it.colors, 10, oriented, "v3")
        _same_dicts(r["car_statistics"], per_frame, why)
        _same_dicts(r["car_statistics"], R.v3_statistics(f["points"], f["lists"], it.bboxes_3d, it.colors, 10, oriented), why)
        for k in ("valid_indices", "count_mb", "n_valid", "bg_assigned", "points_valid"):        # the rest is run_frames'
            assert np.array_equal(r[k], b[k]), why + (k,)
        n += len(per_frame)
    assert n >= 30
    clouds = pipeline.inside_outside_cloud_frames(got)
    for c, r, it, f in zip(clouds, got, items, frames):
        vi = f["g"].get("valid_idx_d%d" % dmax)                 # (frame 2717's file holds its points only)
        ref = R.cloud(R.v3_statistics(f["points"], f["lists"], it.bboxes_3d, it.colors, 10, oriented),
                      f["points"][vi, :3] if vi is not None else r["points_valid"], r["bg_assigned"])
        for k in ("points", "colors", "parts"):
            assert c[k].dtype == ref[k].dtype and np.array_equal(c[k], ref[k]), (tag, f["frame"], k)
        assert c["frame"] == f["frame"] and len(c["points"]) == len(r["valid_indices"]) - int(r["bg_assigned"].sum()) + int(
            sum(d["total_points"] for d in r["car_statistics"]))


def test_statistics_beyond_32_and_256_masks(cal):
    cam = _camera(cal["calib"])
    T = cal["calib"]["TrVeloToRect"]
    g = load_golden(100)
    pts, corners = g["points"][::3], g["corners_velo"]
    for M in (40, 260):
        masks = _wide_masks(M, M, cal["W"], cal["H"])
        it = pipeline.FrameInputs(100, pts, masks, _boxes(corners), pipeline.default_colors(M))
        got = pipeline.car_statistics_v3_frames([it], T, cam, 50.0, 10, True)[0]
        lists = _ref_lists(cal, pts, masks)
        ref = R.v3_statistics(pts, lists, it.bboxes_3d, it.colors, 10, True)
        assert sum(d["matched_bbox_id"] >= 0 for d in ref) >= 3
        _same_dicts(got["car_statistics"], ref, ("M", M))
        c, = pipeline.inside_outside_cloud_frames([got])
        want = R.cloud(ref, got["points_valid"], got["bg_assigned"])
        for k in ("points", "colors", "parts"):
            assert np.array_equal(c[k], want[k]), (M, k)
        assert got["inside_parts"]["off"].shape == (M + 1,) and len(got["inside_parts"]["matched"]) == M


def test_entry_point_default_is_unchanged_and_v3_keys_adds_the_keys(calib, cal, tmp_path, monkeypatch):
    from test_gpu_pipeline import _dataset_tree
    root, seq, cam, velo, gold = _dataset_tree(tmp_path, calib, (100, 570, 1461, 2717, 2939))
    monkeypatch.setattr(pipeline, "sequence_setup", lambda path, s=0, c=0: (seq, cam, calib["TrVeloToCam"], calib["TrVeloToRect"], velo))

    def segmenter(image_path):
        frame = int(os.path.basename(image_path).split(".")[0])
        m = unpack_masks(gold[frame], "edge", cam.height, cam.width)
        return None, m, pipeline.default_colors(len(m)), gold[frame]["boxes2d_edge"], np.ones(len(m))

    def run(**kw):
        seen = []
        with contextlib.redirect_stdout(io.StringIO()) as out:
            res = pipeline.process_frame_with_statistics(0, 0, segmenter=segmenter, image_loader=lambda p: p, kitti360_path=str(root),
                                                         visualizer=lambda f, st, pv, bg: seen.append((f, st, pv, bg)), **kw)
        return res, seen, out.getvalue()
    res, seen, text = run()
    # today's output: run_frames' dicts of the frames with valid points, the summary table printed per frame
    with contextlib.redirect_stdout(io.StringIO()):
        items = pipeline.collect_frame_inputs(str(root), 0, 0, segmenter, lambda p: p, cam, calib["TrVeloToCam"], velo, None)
    want = [r for r in pipeline.run_frames(items, calib["TrVeloToRect"], cam, 50.0, 10, True, 0, False, 0) if r["n_valid"]]
    # (frame 570 has a box file but no visible box: it stays, without statistics; frame 2717 has no box file: dropped)
    assert [r["frame"] for r in res] == [r["frame"] for r in want] == [100, 570, 1461, 2939]
    summary = io.StringIO()
    with contextlib.redirect_stdout(summary):
        for r in want:
            pipeline.print_summary_statistics(r["car_statistics"])
    assert text.endswith(summary.getvalue()) and "SUMMARY STATISTICS" in text
    for a, b, s in zip(res, want, seen):
        assert sorted(a.keys()) == sorted(b.keys()) and "inside_parts" not in a      # (lazy keys appear in the order they were read)
        _same_dicts(a["car_statistics"], b["car_statistics"], (a["frame"],))
        assert all("inside_mask" not in d and "car_points" not in d for d in a["car_statistics"])
        for k in ("valid_indices", "count_mb", "points_valid", "bg_assigned", "u_valid", "v_valid"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        for x, y in zip(a["car_point_sets"], b["car_point_sets"]):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        assert s[0] == a["frame"] and s[1] is a["car_statistics"]
    res3, seen3, text3 = run(v3_keys=True)
    assert text3 == text and [r["frame"] for r in res3] == [100, 570, 1461, 2939]
    for a, b in zip(res3, want):
        per_frame = _quiet(pipeline.calculate_car_point_statistics, b["car_point_sets"], _boxes(gold[a["frame"]]["corners_velo"]),
                           pipeline.default_colors(len(b["car_point_sets"])), 10, True, "v3")
        _same_dicts(a["car_statistics"], per_frame, (a["frame"], "v3"))
        assert "inside_parts" in a


# ---- seeded fuzz ---------------------------------------------------------------------------------------------------------------------
def _axis_box(lo, hi):
    """the 8 corners of [lo, hi] in the dataset's order: c1 - c0, c3 - c0 and c4 - c0 are the box's three edges"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]], np.float64)


def _face_case(seed):
    """Direct cases for the split: per frame boxes with float32-exact corners (some of them twice: ties), points of which many lie
    EXACTLY on slab faces (t = 0 and t = 1 in the reference's quotient), a hair outside them, or anywhere; random ascending lists."""
    rng = np.random.default_rng(seed)
    F, M = int(rng.integers(1, 4)), int(rng.choice([1, 2, 5, 33]))
    frames = []
    for _ in range(F):
        B = int(rng.choice([0, 1, 3, 6]))
        boxes = []
        for _ in range(B):
            lo = rng.integers(-20, 20, 3).astype(np.float64) * 0.25
            boxes.append(_axis_box(lo, lo + rng.integers(1, 12, 3) * 0.25))
        if B >= 3:
            boxes[2] = boxes[0].copy()                           # the same box twice: equal counts, the first one wins
        if B >= 6:                                               # and rotated ones
            boxes[4:6] = list(S.synthetic_boxes(2, seed)[1])
        corners = np.array(boxes).reshape(-1, 8, 3)
        n = int(rng.choice([1, 40, 700, 3000]))
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = rng.uniform(-6, 6, (n, 3))
        for i in range(n):
            if B and rng.random() < 0.7:
                c = corners[int(rng.integers(0, min(B, 4)))]
                lo, hi = c.min(axis=0), c.max(axis=0)
                p = lo + (hi - lo) * rng.integers(0, 5, 3) / 4.0                     # on faces, edges and corners often (0 and 4)
                ax = int(rng.integers(0, 3))
                kind = rng.integers(0, 4)
                if kind == 0:
                    p[ax] = lo[ax]
                elif kind == 1:
                    p[ax] = hi[ax]
                elif kind == 2:
                    p[ax] = np.nextafter(np.float32(hi[ax]), np.float32(np.inf))     # one float32 beyond the face
                pts[i, :3] = p
        lists = [np.sort(rng.choice(n, size=int(rng.integers(0, n + 1)) if rng.random() < 0.8 else 0, replace=False)).astype(np.int64)
                 for _ in range(M)]
        frames.append(dict(points=pts, lists=lists, corners=corners))
    return frames, M, bool(rng.integers(0, 4) > 0)


@pytest.mark.parametrize("seed", range(int(os.environ.get("LPF_FUZZ_CASES", "24"))))
def test_fuzz_faces_ties_and_the_min_points_edge(ctx, cal, seed):
    frames, M, oriented = _face_case(int(os.environ.get("LPF_FUZZ_SEED_BASE", "1000")) + seed)
    base = [R.frame_split(f["points"], f["lists"], f["corners"], 0, oriented) for f in frames]
    best = sorted({int(c) for b in base for c in b["best_cnt"] if c > 0})
    # min_points exactly at a car's best count (it is matched) and one above it (it is not), besides the usual ones
    for mp in sorted({0, 1, 10} | ({best[len(best) // 2], best[len(best) // 2] + 1} if best else set())):
        refs = [R.frame_split(f["points"], f["lists"], f["corners"], mp, oriented) for f in frames]
        if best and mp == best[len(best) // 2]:
            assert any(((r["best_cnt"] == mp) & (r["matched"] == 1)).any() for r in refs)
        if best and mp == best[len(best) // 2] + 1:
            assert any(((r["best_cnt"] == mp - 1) & (r["matched"] == 0)).any() for r in refs)
        cap = max(max(int(r["off"][-1]) for r in refs), 1)
        idx = np.zeros((len(frames), cap), np.int64)
        for i, f in enumerate(frames):
            idx[i, :int(refs[i]["off"][-1])] = np.concatenate(f["lists"]) if M else []
        ctx.set_boxes([f["corners"] for f in frames], oriented=oriented)
        split = ctx.inside_masks([f["points"] for f in frames], idx, np.stack([r["off"] for r in refs]),
                                 np.stack([r["best_box"] for r in refs]), np.stack([r["best_cnt"] for r in refs]), min_points=mp)
        for i, r in enumerate(refs):
            _check_frame(split, i, M, r, (seed, mp, i))


def test_fuzz_has_ties_and_face_points():
    """the generator does what the fuzz is for: cars whose best count two boxes share, and points with t = 0 and t = 1 exactly"""
    ties = faces = 0
    for seed in range(1000, 1024):
        frames, M, oriented = _face_case(seed)
        for f in frames:
            b = R.frame_split(f["points"], f["lists"], f["corners"], 0, oriented)
            hit = (b["count_mb"] == b["best_cnt"][:, None]) & (b["best_cnt"][:, None] > 0)
            ties += int((hit.sum(axis=1) > 1).sum())
            for m in np.flatnonzero(hit.sum(axis=1) > 1):
                assert b["best_box"][m] == int(np.argmax(hit[m]))                    # the first strict maximum
            for c in f["corners"][:4]:
                p = f["points"][:, :3].astype(np.float64) - c[0]
                for e in (c[1] - c[0], c[3] - c[0], c[4] - c[0]):
                    t = np.dot(p, e) / np.dot(e, e)
                    faces += int(((t == 0.0) | (t == 1.0)).sum())
    assert ties > 20 and faces > 1000


@pytest.mark.parametrize("seed", range(int(os.environ.get("LPF_FUZZ_CASES", "24")) // 2))
def test_fuzz_whole_path_against_the_oracle_lists(seed, calib):
    """test_gpu_fuzz's random cases through run_batch and the split: lists from the CPU oracle, the split from the restatement"""
    from test_gpu_fuzz import _case
    T, K, W, H, dmax, oriented, M, frames, masks, boxes = _case(int(os.environ.get("LPF_FUZZ_SEED_BASE", "1000")) + 500 + seed, calib)
    mp = (0, 1, 3, 10)[seed % 4]
    with LpfContext(0) as c:
        c.set_camera(T, K, W, H, 0.0, dmax)
        c.set_masks(np.stack(masks))
        c.set_boxes(boxes, oriented=oriented)
        staged = c.stage_points(frames)
        res = c.run_batch(frames, want_uv=False, want_label=False, staged=staged)
        split = c.inside_masks(None, *pipeline.inside_list_arrays(res, M), min_points=mp, staged=staged)
    for f, r in enumerate(res):
        lab = orc.pack_masks(masks[f], 0, H, W) if M else None
        o = orc.run(frames[f], T, K, W, H, 0.0, dmax, label_img=lab, M=M, corners=boxes[f], oriented=oriented, want_float=False)
        ref = R.frame_split(frames[f], o["inst_lists"], boxes[f], mp, oriented)
        assert np.array_equal(ref["count_mb"], o["count_mb"].reshape(ref["count_mb"].shape)) and np.array_equal(ref["best_box"], o["best_box"])
        _check_frame(split, f, M, ref, (seed, f), r["count_mb"])
