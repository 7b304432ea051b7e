"""lpf_match_2d / LpfContext.match_2d / match_detections_frames / improved_match_detections_frames on the GPU: every output against the
NumPy restatement of the reference's arithmetic (tests/match2d_ref.py, held against the scalar functions in tests/test_match2d_api.py)
bit for bit, and against the goldens the reference's own functions produced (tests/golden/match2d_golden.npz)."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

import match2d_ref as R
from conftest import GOLDEN, golden_frames, load_golden
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd._native import SUMMARY_DTYPE, LpfContext, Match2dInput, Match2dOutputs
from test_match2d_api import compare_with_golden, golden_frame

pytestmark = pytest.mark.gpu
MATS = ("iou", "center", "size", "total", "cost")
ALL = ("best",) + MATS


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(GOLDEN, "match2d_golden.npz"))
    return {f: golden_frame(z, f) for f in z["frames"].tolist()}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _check_frame(res, f, dets, bb, front, what, min_iou=0.25, weights=(0.5, 0.3, 0.2), keys=ALL):
    """frame f of a match_2d result against the restatement, bit for bit; returns the restatement's outputs"""
    exp = R.match(dets, bb, front, min_iou, weights)
    for k in keys:
        if k == "best":
            assert np.array_equal(_host(res["best_box"][f]), exp["best_box"]), (what, "best_box")
            assert R.same_bits(_host(res["best_iou"][f]), exp["best_iou"]), (what, "best_iou")
        else:
            got = _host(res[k][f])
            assert got.shape == exp[k].shape, (what, k)
            assert R.same_bits(got, exp[k]), (what, k, int((got != exp[k]).sum()), float(np.abs(got - exp[k]).max()))
    return exp


# ---- 5. the golden frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_golden_frames_in_one_batch_and_frame_by_frame(ctx, gold, where, dtype):
    frames = sorted(gold)
    dets = [gold[f]["dets"].astype(dtype) for f in frames]
    bbs = [gold[f]["bbox2d"].astype(np.float64) for f in frames]
    fronts = [gold[f]["front"].astype(np.int32) for f in frames]
    put = _dev if where == "device" else (lambda a: a)
    batch = ctx.match_2d([put(d) for d in dets], [put(b) for b in bbs], [put(f) for f in fronts], want=ALL)
    if where == "device":
        import torch
        torch.cuda.synchronize()
        assert all(t.is_cuda for t in batch["cost"])
    n_hit = 0
    for k, f in enumerate(frames):
        exp = _check_frame(batch, k, dets[k], bbs[k], fronts[k], (f, "batch"))
        n_hit += int((exp["iou"] > 0).sum())
        one = ctx.match_2d([put(dets[k])], [put(bbs[k])], [put(fronts[k])], want=ALL)
        _check_frame(one, 0, dets[k], bbs[k], fronts[k], (f, "alone"))
        if dtype is np.float32:                              # the reference's own numbers
            got = {m: _host(batch[m][k]) for m in MATS}
            compare_with_golden(got, gold[f], "frame %d" % f)
            assert np.array_equal(_host(batch["best_box"][k]), gold[f]["v4_best"]), f
    assert n_hit > 1000


# ---- 6. the square root -------------------------------------------------------------------------------------------------------
def test_centre_distance_is_the_correctly_rounded_root_of_the_fused_sum(ctx):
    """10^6 seeded centre offsets with |dx|, |dy| < 700 (the centre score is not clamped), half of them multiples of 0.5 as real
    centres are: 1000 frames of one detection centred at the origin against 1000 boxes each."""
    rng = np.random.default_rng(20261016)
    F, B = 1000, 1000
    off = rng.uniform(-699.0, 699.0, (F, B, 2))
    off[:, ::2] = np.round(off[:, ::2] * 2.0) / 2.0
    half = rng.integers(1, 40, (F, B, 2)).astype(np.float64)
    half[:, 1::2] += rng.random((F, B // 2, 2))
    bbs = [np.concatenate([-off[f] - half[f], -off[f] + half[f]], axis=1) for f in range(F)]
    dets = [np.array([[-8.0, -6.0, 8.0, 6.0]], np.float64)] * F
    fronts = [np.full(B, 8, np.int32)] * F
    res = ctx.match_2d(dets, bbs, fronts, want=("center", "cost"))
    bad = worst = 0
    n_half = 0
    for f in range(F):
        exp = R.score(dets[f], bbs[f], fronts[f])
        got = res["center"][f]
        bad += int((got.view(np.int64) != exp["center"].view(np.int64)).sum())
        worst = max(worst, float(np.abs(got - exp["center"]).max()))
        assert (exp["center"] > 0).all()                     # never clamped
        cx = (bbs[f][:, 0] + bbs[f][:, 2]) / 2
        n_half += int((cx * 2 == np.round(cx * 2)).sum())
        assert R.same_bits(res["cost"][f], exp["cost"]), f
    print("centre scores that differ: %d of %d (largest difference %g); offsets on the half-pixel grid: %d" % (bad, F * B, worst, n_half))
    assert n_half >= F * B // 2
    assert bad == 0, (bad, worst)


# ---- 7. sizes and shapes --------------------------------------------------------------------------------------------------------
def _sweep_shapes():
    Ds, Bs = (0, 1, 3, 4, 5, 256, 300), (0, 1, 63, 64, 65, 314, 1000)
    shapes = [(Ds[i % 7], Bs[i // 7]) for i in range(49)]                                     # every combination once
    shapes += [((256, 300)[i % 2], (314, 1000, 65, 314)[i % 4]) for i in range(146 - 49)]       # then crowded frames
    return shapes


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ragged_sizes_over_146_frames(ctx, dtype):
    shapes = _sweep_shapes()
    assert len(shapes) == 146 and sum(d * b for d, b in shapes) > 8_000_000
    # five float64 matrices of a host caller are more than lpf_match_2d stages at once (256 MiB): `full` goes through in two ranges of
    # frames.  (The split is not observed here: a kernel trace of this case shows two lpf_m2_pairs launches for `full`.)
    assert sum(d * b for d, b in shapes) * 5 * 8 > (256 << 20)
    data = [R.cases(1000 + i, d, b, dtype, fraction=bool(i % 2)) for i, (d, b) in enumerate(shapes)]
    dets, bbs, fronts = [x[0] for x in data], [x[1] for x in data], [x[2] for x in data]
    full = ctx.match_2d(dets, bbs, fronts, min_iou=0.1, want=ALL)
    only_best = ctx.match_2d(dets, bbs, fronts, min_iou=0.1, want=("best",))
    only_cost = ctx.match_2d(dets, bbs, fronts, min_iou=0.1, want=("cost",))
    assert set(only_best) == {"best_box", "best_iou"} and set(only_cost) == {"cost"}
    n_pairs = n_hit = 0
    for f in range(len(shapes)):
        exp = _check_frame(full, f, dets[f], bbs[f], fronts[f], ("sweep", f, shapes[f]), min_iou=0.1)
        assert np.array_equal(only_best["best_box"][f], full["best_box"][f]) and R.same_bits(only_best["best_iou"][f], full["best_iou"][f])
        assert R.same_bits(only_cost["cost"][f], full["cost"][f])
        n_pairs += exp["iou"].size
        n_hit += int((exp["iou"] > 0).sum())
    print("pairs %d, with IoU > 0 %d" % (n_pairs, n_hit))
    assert n_hit * 4 >= n_pairs


def test_device_tensors_other_weights_and_a_batch_of_nothing(ctx):
    import torch
    shapes = [(5, 65), (0, 10), (7, 0), (300, 1000), (3, 4)]
    data = [R.cases(77 + i, d, b, np.float32, True) for i, (d, b) in enumerate(shapes)]
    w = (0.25, 0.5, 0.125)
    res = ctx.match_2d([_dev(x[0]) for x in data], [_dev(x[1]) for x in data], [_dev(x[2]) for x in data], min_iou=-1.0, weights=w, want=ALL)
    torch.cuda.synchronize()
    for f, x in enumerate(data):
        _check_frame(res, f, *x, ("device", f), min_iou=-1.0, weights=w)
    assert _host(res["best_box"][2]).tolist() == [-1] * 7 and not _host(res["best_iou"][2]).any()
    res = ctx.match_2d([], [], [], want=ALL)
    assert all(res[k] == [] for k in res)
    res = ctx.match_2d([np.zeros((0, 4), np.float32)], [data[0][1]], [data[0][2]], want=ALL)
    assert res["cost"][0].shape == (0, 65) and res["best_box"][0].shape == (0,)


def test_raw_call_refusals(ctx):
    dets, bb, front = R.cases(5, 4, 6, np.float32)
    det_off, box_off = np.array([0, 4], np.int32), np.array([0, 6], np.int32)
    best = np.zeros(4, np.int32)

    def call(F=1, d=True, b=True, f=True, doff=det_off, boff=box_off, min_iou=0.25, w=0.5, inp=True, out=True):
        i, o = Match2dInput(), Match2dOutputs()
        i.dets, i.bbox2d, i.front = (dets.ctypes.data if d else None), (bb.ctypes.data if b else None), (front.ctypes.data if f else None)
        i.det_off, i.box_off = (None if doff is None else doff.ctypes.data), (None if boff is None else boff.ctypes.data)
        i.min_iou, i.w_iou, i.w_center, i.w_size = min_iou, w, 0.3, 0.2
        o.best_box = best.ctypes.data
        return ctx._lib.lpf_match_2d(ctx._h, F, ctypes.byref(i) if inp else None, ctypes.byref(o) if out else None)
    assert call() == 0
    assert call(F=-1) == -1 and call(inp=False) == -1 and call(out=False) == -1
    assert call(doff=None) == -1 and call(boff=None) == -1
    assert call(doff=np.array([4, 0], np.int32)) == -1 and call(boff=np.array([6, 5], np.int32)) == -1
    assert call(doff=np.array([-1, 3], np.int32)) == -1
    assert call(d=False) == -1 and call(b=False) == -1 and call(f=False) == -1
    assert call(min_iou=float("nan")) == -1 and call(w=float("inf")) == -1
    assert "finite" in (ctx._lib.lpf_last_error(ctx._h) or b"").decode()
    assert call(F=0) == 0
    assert call(b=False, f=False, boff=np.array([0, 0], np.int32)) == 0           # a frame without boxes needs no box arrays
    assert best.tolist() == [-1] * 4


# ---- 8. the pipeline's batched matchers against the scalar ones ---------------------------------------------------------------------
def _camera(calib):
    return kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))


def _same_lists(got, exp, what):
    assert len(got) == len(exp), what
    for (gc, gcol), (ec, ecol) in zip(got, exp):
        assert type(gc) is type(ec) and gc.dtype == ec.dtype and np.array_equal(gc, ec), what
        assert type(gcol) is type(ecol) and np.array_equal(np.asarray(gcol), np.asarray(ecol)), what
        if isinstance(ecol, np.ndarray):
            assert gcol.dtype == ecol.dtype, what


def test_batched_matchers_equal_the_scalar_ones_on_the_sample_frames(calib, gold):
    cam = _camera(calib)
    dets, boxes, frames = [], [], []
    for r in golden_frames()["frames"]:
        f = r["frame"]
        frames.append(f)
        if "skipped" in r:                                   # the sample's frame without a box file: an empty frame
            dets.append(np.zeros((0, 4), np.float32))
            boxes.append([])
            continue
        g = load_golden(f)
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        boxes.append(list(pipeline.prepare_boxes(raw, cam, calib["TrVeloToCam"], keep_all=True)))
        dets.append(gold[f]["dets"])
        assert len(boxes[-1]) == len(gold[f]["bbox2d"])
    assert len(frames) == 20 and sum(1 for b in boxes if not b) == 1
    for b in boxes[1]:                                       # dicts that were not made by prepare_boxes: projected by the batch call
        del b["_bbox2d"], b["_front"]
    for b in boxes[3][::3]:
        del b["_bbox2d"], b["_front"]
    for b in boxes[2][1::2]:                                 # never transformed: matched, but nothing to return
        del b["corners_velo"]
    for b in boxes[4][:5]:                                   # no cam-0 corners: both matchers skip the box
        del b["corners_cam0"]
    dets[5] = dets[5].astype(np.float64)                     # a frame whose detections are float64
    colors4 = [pipeline.generate_consistent_colors(len(d)) for d in dets]
    colors5 = [pipeline.generate_consistent_colors(max(len(d) - 2, 0)) for d in dets]      # more detections than colours: V5's red
    got4 = pipeline.match_detections_frames(dets, boxes, colors4, cam)
    got4_low = pipeline.match_detections_frames(dets, boxes, colors4, cam, min_iou=0.1)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got5 = pipeline.improved_match_detections_frames(dets, boxes, colors5, cam)
    exp_out = io.StringIO()
    n4 = n5 = 0
    for k, f in enumerate(frames):
        _same_lists(got4[k], pipeline.match_detections_to_bboxes(dets[k], boxes[k], colors4[k], cam), (f, "V4"))
        _same_lists(got4_low[k], pipeline.match_detections_to_bboxes(dets[k], boxes[k], colors4[k], cam, min_iou=0.1), (f, "V4 0.1"))
        with contextlib.redirect_stdout(exp_out):
            exp5 = pipeline.improved_match_detections_to_bboxes(dets[k], boxes[k], colors5[k], cam)
        _same_lists(got5[k], exp5, (f, "V5"))
        n4 += len(got4[k])
        n5 += sum(1 for p in got5[k] if isinstance(p[1], np.ndarray))
    assert out.getvalue() == exp_out.getvalue()
    assert n4 > 40 and n5 > 40 and "Rejected match" in out.getvalue() and "No detections or 3D bounding boxes" in out.getvalue()
    # untouched frames: the reference's own lists
    for k, f in enumerate(frames):
        if k in (1, 2, 3, 4, 5) or f not in gold:
            continue
        assert np.array_equal(np.array([p[0] for p in got4[k]]).reshape(-1, 8, 3), gold[f]["v4_corners"]), f
        assert np.array_equal(np.array([p[0] for p in got5[k]]).reshape(-1, 8, 3), gold[f]["v5_corners"]), f


# ---- 9. conventions -----------------------------------------------------------------------------------------------------------------
def test_refuses_capture_and_leaves_the_state(calib):
    import overlay_ref as O
    H, W = int(calib["height"]), int(calib["width"])
    fr = O.golden_inputs(H, W)["100"]
    g = load_golden(100)
    dets, bb, front = R.cases(9, 12, 40, np.float32, True)
    with LpfContext(0) as c:
        assert set(c.match_2d([dets], [bb], [front], want=("best",))) == {"best_box", "best_iou"}      # no camera, masks or boxes needed
        c.set_camera(np.asarray(calib["TrVeloToRect"], np.float64), np.asarray(calib["K"], np.float64)[:3, :3], W, H, 0.0, 30.0)
        c.set_masks(fr["rect5"])
        c.set_boxes([g["corners_velo"]])
        before = c.run(fr["pts"], want_float=True)
        ref = c.match_2d([dets], [bb], [front], want=ALL)
        after = c.run(fr["pts"], want_float=True)
        n = 0
        for k, v in before.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, after[k]), k
                n += 1
        assert n >= 5 and before["count_mb"].any()
        c.graph_begin()
        i, o = Match2dInput(), Match2dOutputs()
        det_off, box_off = np.array([0, len(dets)], np.int32), np.array([0, len(bb)], np.int32)
        out = np.full(len(dets), 7, np.int32)
        i.dets, i.bbox2d, i.front, i.det_off, i.box_off = dets.ctypes.data, bb.ctypes.data, front.ctypes.data, det_off.ctypes.data, box_off.ctypes.data
        i.min_iou, i.w_iou, i.w_center, i.w_size = 0.25, 0.5, 0.3, 0.2
        o.best_box = out.ctypes.data
        assert c._lib.lpf_match_2d(c._h, 1, ctypes.byref(i), ctypes.byref(o)) == -3
        assert "captured" in (c._lib.lpf_last_error(c._h) or b"").decode()
        assert (out == 7).all()
        again = c.match_2d([dets], [bb], [front], want=ALL)
        for k in ref:
            assert np.array_equal(again[k][0], ref[k][0]), k
        last = c.run(fr["pts"], want_float=True)
        for k, v in before.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, last[k]), k


def test_pipelined_steps_around_a_device_call(calib):
    import torch
    import overlay_ref as O
    H, W = int(calib["height"]), int(calib["width"])
    T, K = np.asarray(calib["TrVeloToRect"], np.float64), np.asarray(calib["K"], np.float64)[:3, :3]
    inputs = O.golden_inputs(H, W)
    order = ["100", "full_1461", "full_2449"]

    def steps(c, keep):
        outs = []
        for k in order:
            fr = inputs[k]
            n = len(fr["pts"])
            dp, dm, dr = _dev(fr["pts"]), _dev(fr["rect5"]), _dev(LpfContext.mask_rects(fr["rect5"]))
            no = dict(uv=torch.empty((n, 2), dtype=torch.int32, device="cuda"), label_bits=torch.empty(n, dtype=torch.int32, device="cuda"),
                      valid_idx=torch.empty(n, dtype=torch.int64, device="cuda"), inst_idx=torch.empty((1, n), dtype=torch.int64, device="cuda"),
                      summary=torch.empty(SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda"))
            for t in no.values():
                t.view(torch.uint8).fill_(0xA5)
            keep.append((dp, dm, dr, no))
            outs.append((c.make_frame_step(dp, masks_u8=dm, mask_rects=dr, inst_cap=n, **no), no))
        return outs

    data = [R.cases(300 + i, d, b, np.float32, True) for i, (d, b) in enumerate([(40, 314), (5, 25), (256, 600)])]
    dev = [[_dev(x[k]) for x in data] for k in range(3)]
    keep = []
    with LpfContext(0) as ref:
        ref.set_camera(T, K, W, H, 0.0, 30.0)
        want = []
        for step, no in steps(ref, keep):
            step()
            ref.sync()
            want.append({k: t.cpu().numpy().copy() for k, t in no.items()})
    with LpfContext(0) as c:
        c.set_pipelined("fused-pack")
        c.set_camera(T, K, W, H, 0.0, 30.0)
        jobs = steps(c, keep)
        for step, _ in jobs:
            step()
        c.sync()
        res = c.match_2d(*dev, want=ALL)                     # (first use: the context's buffers are allocated)
        c.sync()
        for step, _ in jobs:
            step()
        s0 = c.stats()
        res = c.match_2d(*dev, want=ALL)                     # the pipeline's owed launches go first; nothing waits
        s1 = c.stats()
        assert s1["host_waits"] == s0["host_waits"] and s1["blocking_uploads"] == s0["blocking_uploads"], (s0, s1)
        assert s1["drains"] == s0["drains"] + 1 and s1["uploads"] > s0["uploads"]
        for step, _ in jobs:                                 # later steps are unchanged
            step()
        c.sync()
        torch.cuda.synchronize()
        for (_, no), w in zip(jobs, want):
            for k, t in no.items():
                assert np.array_equal(t.cpu().numpy(), w[k]), k
    for f, x in enumerate(data):
        _check_frame(res, f, *x, ("pipelined", f))
