#!/usr/bin/env python3
"""The 2D matching of detections to projected boxes (V4:140-183, V5:307-416) for a batch of frames, two routes:
  scalar   pipeline.match_detections_to_bboxes (V4) / pipeline.improved_match_detections_to_bboxes (V5) once per frame: the parent's
           interpreted double loops, '_bbox2d' already in the box dicts, prints swallowed.  Timed on one frame per distinct box set
           and scaled to the batch (a 146-frame batch of 256 x 314 pairs would take minutes)
  batched  LpfContext.match_2d: one lpf_match_2d call for the batch, want = ("best",) for V4, every matrix for V5 -- device-resident
           (GPU tensors in and out, timed to completion) and NumPy in / NumPy out; and the whole pipeline functions
           match_detections_frames / improved_match_detections_frames (pair stage + the Python around it + scipy's assignment)
Batch: the boxes of the four full-size golden frames (100, 1461, 2098, 2449: 31, 21, 186 and 314 annotated boxes) in turn to 146
frames, with 5, 32 and 256 float32 detections per frame made by a seeded rule from the boxes' own projections.
Appends one JSON line per (route, mode, detections) with the library's build id.
  python tools/match2d_bench.py [--dets 5,32,256] [--passes 20] [--out profiles/match2d_bench.jsonl]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
BOX_FILES = ("frame_0000000100", "frame_0000001461_full", "frame_0000002098_full", "frame_0000002449_full")
FRAMES = 146
ALL = ("iou", "center", "size", "total", "cost")


class Cam:
    def __init__(self, calib):
        self.K, self.width, self.height = np.asarray(calib["K"], np.float64)[:3, :3], int(calib["width"]), int(calib["height"])


def detections(seed, n, bb, front, W, H):
    """n float32 detections: projections of boxes that reach into the image, clipped and jittered; every eighth one unrelated"""
    rng = np.random.default_rng(seed)
    inside = np.flatnonzero((front > 0) & (bb[:, 0] < W) & (bb[:, 2] > 0) & (bb[:, 1] < H) & (bb[:, 3] > 0))
    out = np.zeros((n, 4))
    for i in range(n):
        if i % 8 == 7 or not len(inside):
            a, b = rng.uniform(0, W - 60), rng.uniform(0, H - 40)
            out[i] = [a, b, a + rng.uniform(10, 300), b + rng.uniform(10, 150)]
        else:
            r = np.clip(bb[rng.choice(inside)], [0, 0, 0, 0], [W - 1, H - 1, W - 1, H - 1])
            out[i] = r + rng.normal(0, 4, 4)
    return out.astype(np.float32)


def timed(fn, passes, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", default="5,32,256")
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match2d_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from lidar_object_detection_amd import _build, pipeline
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    cam = Cam(calib)
    ctx = pipeline.get_context(0)
    sets = []
    for name in BOX_FILES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        boxes = list(pipeline.prepare_boxes(raw, cam, calib["TrVeloToCam"], keep_all=True))
        bb = np.array([b["_bbox2d"] if b["_bbox2d"] is not None else [0.0] * 4 for b in boxes], np.float64)
        front = np.array([b["_front"] for b in boxes], np.int32)
        sets.append((boxes, bb, front))
    lines = []

    def emit(**kw):
        kw["source_id"] = _build.library_id(_build.LIB)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    for D in (int(x) for x in a.dets.split(",")):
        which = [f % len(sets) for f in range(FRAMES)]
        dets = [detections(9000 + f, D, sets[k][1], sets[k][2], cam.width, cam.height) for f, k in enumerate(which)]
        boxes = [sets[k][0] for k in which]
        bbs, fronts = [sets[k][1] for k in which], [sets[k][2] for k in which]
        colors = pipeline.generate_consistent_colors(D)
        pairs = sum(len(d) * len(b) for d, b in zip(dets, bbs))
        base = dict(frames=FRAMES, dets_per_frame=D, pairs=pairs)
        # scalar: one frame per box set, scaled
        for mode, fn in (("v4", pipeline.match_detections_to_bboxes), ("v5", pipeline.improved_match_detections_to_bboxes)):
            per_set = []
            with contextlib.redirect_stdout(io.StringIO()):
                fn(dets[0][:2], boxes[0], colors, cam)        # (untimed: the first call imports scipy.optimize)
            for k in range(len(sets)):
                f = which.index(k)
                with contextlib.redirect_stdout(io.StringIO()):
                    t0 = time.perf_counter()
                    fn(dets[f], boxes[f], colors, cam)
                    per_set.append((time.perf_counter() - t0) * 1e3)
            emit(route="scalar", mode=mode, ms_per_batch_scaled=round(sum(per_set[k] for k in which), 3),
                 ms_per_frame_by_box_set=[round(t, 3) for t in per_set], timed_frames=len(sets), **base)
        # batched: the native call
        dev = [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrs] for arrs in (dets, bbs, fronts)]
        for mode, want in (("v4", ("best",)), ("v5", ALL)):
            def on_device():
                ctx.match_2d(*dev, want=want)
                torch.cuda.synchronize()
            med, lo, hi = timed(on_device, a.passes, a.warmup)
            emit(route="batched", mode=mode, where="device", ms_per_batch_median=round(med, 3), ms_per_batch_min=round(lo, 3), ms_per_batch_max=round(hi, 3),
                 pairs_per_s=round(pairs / (lo * 1e-3)), passes=a.passes, **base)
            med, lo, hi = timed(lambda: ctx.match_2d(dets, bbs, fronts, want=want), a.passes, a.warmup)
            emit(route="batched", mode=mode, where="numpy", ms_per_batch_median=round(med, 3), ms_per_batch_min=round(lo, 3), ms_per_batch_max=round(hi, 3),
                 pairs_per_s=round(pairs / (lo * 1e-3)), passes=a.passes, **base)
        # batched: the pipeline functions, lists and printed lines included
        med, lo, hi = timed(lambda: pipeline.match_detections_frames(dets, boxes, [colors] * FRAMES, cam, ctx=ctx), max(a.passes // 4, 3), 1)
        emit(route="batched", mode="v4", where="pipeline", ms_per_batch_median=round(med, 3), ms_per_batch_min=round(lo, 3), ms_per_batch_max=round(hi, 3), **base)

        def v5_frames():
            with contextlib.redirect_stdout(io.StringIO()):
                pipeline.improved_match_detections_frames(dets, boxes, [colors] * FRAMES, cam, ctx=ctx)
        med, lo, hi = timed(v5_frames, max(a.passes // 4, 3), 1)
        emit(route="batched", mode="v5", where="pipeline", ms_per_batch_median=round(med, 3), ms_per_batch_min=round(lo, 3), ms_per_batch_max=round(hi, 3), **base)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
