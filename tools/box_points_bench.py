#!/usr/bin/env python3
"""Per-box LiDAR point counts, first boxes and point-level confusion counts for a batch of real frames, two routes:
  (a) per-frame  run_frames, then one blocking lpf_points_in_boxes call per frame on the frame's valid points, which brings the
                 [B][n_valid] byte matrix back to be summed per box, reduced to a first box per point (argmax) and crossed with the
                 labels in NumPy -- the only route to these numbers before lpf_box_points.  Its per-frame part is timed on one frame
                 per distinct scan and scaled to the batch (every 4th frame of the batch is the same scan)
  (b) batched    pipeline.point_recall_frames: the same pass plus ONE lpf_box_points call for the batch
  (c) kernel     --kernel-only: the pass once, then lpf_box_points alone on device-resident points, lists and outputs, for one
                 `rocprofv3 --kernel-trace --stats` run of its own; --from-stats DIR turns that run into the kernel's time, its box
                 tests per second and its bytes (per valid point 8 index + 16 point + 4 label read, 4 written) against HBM's peak
Batch A: 146 frames, the four full-size golden frames (100, 1461, 2098, 2449: 16.9 M points) in turn, their five masks and their
visible boxes.  Batch R: the same frames with ALL raw boxes kept (up to 314 per frame: several box tiles).  One JSON line per
(batch, route) with the library's build id, appended to --out.
  python tools/box_points_bench.py [--batches A,R] [--passes 7] [--out profiles/box_points_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/box_points_bench.py --kernel-only A [--calls 20]
  python tools/box_points_bench.py --from-stats DIR --kernel-only A --tests N --valid N"""
import argparse
import contextlib
import csv
import glob
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
NAMES = ("frame_0000000100", "frame_0000001461_full", "frame_0000002098_full", "frame_0000002449_full")
FRAMES = 146
BYTES_PER_VALID = 8 + 16 + 4 + 4
HBM_PEAK = 8e12


class Cam:
    def __init__(self, calib):
        self.K, self.width, self.height = np.asarray(calib["K"], np.float64)[:3, :3], int(calib["width"]), int(calib["height"])


def batch(which, calib):
    """FrameInputs of batch A (visible boxes) or R (all raw boxes): the four scans in turn, five masks per frame"""
    from lidar_object_detection_amd import pipeline
    cam = Cam(calib)
    scans = []
    for name in NAMES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        masks = np.ascontiguousarray(np.unpackbits(g["masks_rect5_packed"], axis=-1)[..., :cam.width].astype(np.uint8))
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        with contextlib.redirect_stdout(io.StringIO()):
            boxes = pipeline.prepare_boxes(raw, cam, calib["TrVeloToCam"], keep_all=which == "R", as_arrays=True)
        scans.append((np.ascontiguousarray(g["points"], dtype=np.float32), masks, boxes))
    colors = pipeline.default_colors(5)
    return [pipeline.FrameInputs(f, *scans[f % 4], colors) for f in range(FRAMES)], cam


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), passes=len(ts))


def per_frame(ctx, r, item):
    """route (a)'s part of one frame: the byte matrix of its valid points against its boxes, then the sums in NumPy"""
    from lidar_object_detection_amd import pipeline
    corners, _ = pipeline._corners_velo(item.bboxes_3d)
    inside = ctx.points_in_boxes(r["points_valid"], corners, True)
    lab = r["bg_assigned"]
    anyb = inside.any(axis=0)
    first = np.where(anyb, inside.argmax(axis=0), -1).astype(np.int32)
    return dict(box_points=inside.sum(axis=1).astype(np.int32), box_labelled=(inside & lab[None, :]).sum(axis=1).astype(np.int32), first_box=first,
                frame_counts=np.array([len(lab), anyb.sum(), lab.sum(), (anyb & lab).sum()], np.int64))


def end_to_end(which, calib, passes, warmup):
    from lidar_object_detection_amd import pipeline
    items, cam = batch(which, calib)
    T = np.asarray(calib["TrVeloToRect"])
    ctx = pipeline.get_context(0)
    ta, ts4, tb = [], [[] for _ in range(4)], []
    for p in range(warmup + passes):                         # the two routes in turn, pass by pass
        t0 = time.perf_counter()
        res = pipeline.run_frames(items, T, cam, 50.0, 10, True, ctx=ctx)
        t1 = time.perf_counter()
        per, want = [], []
        for f in range(4):                                   # the per-frame part of one frame per distinct scan
            t2 = time.perf_counter()
            want.append(per_frame(ctx, res[f], items[f]))
            per.append((time.perf_counter() - t2) * 1e3)
        t3 = time.perf_counter()
        got = pipeline.point_recall_frames(items, T, cam, 50.0, 10, True, ctx=ctx)
        t4 = time.perf_counter()
        if p == 0:                                           # the two routes agree (first frame of each scan)
            for f in range(4):
                c = got[f]["point_confusion"]
                fc = want[f]["frame_counts"]
                assert [c["tp"], c["fp"], c["fn"], c["tn"]] == [fc[3], fc[2] - fc[3], fc[1] - fc[3], fc[0] - fc[1] - fc[2] + fc[3]]
                for k in ("box_points", "box_labelled", "first_box"):
                    assert np.array_equal(got[f][k], want[f][k]), (f, k)
        if p >= warmup:
            ta.append((t1 - t0) * 1e3)
            for f in range(4):
                ts4[f].append(per[f])
            tb.append((t4 - t3) * 1e3)
    valid = int(sum(r["n_valid"] for r in got))
    tests = int(sum(r["n_valid"] * len(r["box_points"]) for r in got))
    base = dict(batch=which, frames=FRAMES, valid_points=valid, box_tests=tests, boxes_per_scan=[len(items[f].bboxes_3d) for f in range(4)],
                points_in_a_box=int(sum(r["point_confusion"]["tp"] + r["point_confusion"]["fn"] for r in got)))
    n_of = [sum(1 for f in range(FRAMES) if f % 4 == k) for k in range(4)]
    scaled = [sum(n_of[k] * ts4[k][i] for k in range(4)) for i in range(passes)]
    total_a = [x + y for x, y in zip(ta, scaled)]
    return [dict(route="a_per_frame", run_frames=spread(ta), per_frame_scaled=spread(scaled), total=spread(total_a),
                 per_frame_ms_by_scan=[round(statistics.median(t), 3) for t in ts4], **base),
            # (the two routes ran in turn: pass by pass the difference is taken on the same state of the host)
            dict(route="b_batched", total=spread(tb), beyond_run_frames_ms_median=round(statistics.median(tb) - statistics.median(ta), 2),
                 a_minus_b_pass_by_pass=spread([x - y for x, y in zip(total_a, tb)]), **base)]


def kernel_only(which, calib, calls):
    """the pass once, then lpf_box_points `calls` times on device-resident points, lists and outputs (all four outputs)"""
    import torch
    from lidar_object_detection_amd import pipeline
    items, cam = batch(which, calib)
    ctx = pipeline.get_context(0)
    ctx.set_camera(np.asarray(calib["TrVeloToRect"]), cam.K, cam.width, cam.height, 0.0, 50.0)
    stacks, _, _ = pipeline._frame_mask_stacks(items, cam, ctx, 0, False)
    staged = ctx.stage_points([f.points for f in items])
    res, _ = pipeline._frames_pass(items, stacks, 5, cam, True, 0, False, ctx, staged=staged)
    off = staged[0]
    valid, labels = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.int32)
    n_valid = np.array([r["n_valid"] for r in res], np.int64)
    for i, r in enumerate(res):
        valid[off[i]:off[i] + n_valid[i]] = r["valid_idx"]
        labels[off[i]:off[i] + n_valid[i]] = r["label_valid"].view(np.int32)
    lists = [torch.from_numpy(a).cuda() for a in (valid, n_valid, labels)]
    Btot = int(ctx.box_off[-1])
    out = dict(box_points=torch.zeros(Btot, dtype=torch.int32, device="cuda"), box_labelled=torch.zeros(Btot, dtype=torch.int32, device="cuda"),
               first_box=torch.full((int(off[-1]),), -1, dtype=torch.int32, device="cuda"),
               frame_counts=torch.zeros((FRAMES, 4), dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        ctx.box_points(None, *lists, out=out, staged=staged)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / calls
    tests = int(sum(int(n) * int(ctx.box_off[i + 1] - ctx.box_off[i]) for i, n in enumerate(n_valid)))
    return dict(route="c_kernel_only", batch=which, frames=FRAMES, valid_points=int(n_valid.sum()), boxes=Btot, box_tests=tests, calls=calls,
                host_ms_per_call=round(ms, 3), bytes_per_valid_point=BYTES_PER_VALID, points_in_a_box=int(out["frame_counts"][:, 1].sum()),
                box_points_total=int(out["box_points"].sum()))


def from_stats(dirs, which, tests, valid):
    w = csv.writer(sys.stdout)
    w.writerow(["batch", "kernel", "calls", "avg_us", "min_us", "max_us", "box_tests", "Gtests_per_s", "valid_points", "bytes_per_valid_point", "GBps",
                "of_8TBps_peak"])
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not f:
            continue
        for r in csv.DictReader(open(f[-1])):
            if "lpf_box_points_kernel" not in r["Name"]:
                continue
            avg = float(r["AverageNs"]) / 1e3
            bps = valid * BYTES_PER_VALID / (avg * 1e-6)
            w.writerow([which, r["Name"], r["Calls"], "%.2f" % avg, "%.2f" % (float(r["MinNs"]) / 1e3), "%.2f" % (float(r["MaxNs"]) / 1e3),
                        tests, "%.1f" % (tests / (avg * 1e-6) / 1e9), valid, BYTES_PER_VALID, "%.1f" % (bps / 1e9), "%.4f" % (bps / HBM_PEAK)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="A,R")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", metavar="BATCH")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--tests", type=int, default=0, help="--from-stats: box tests per call (the kernel-only line's box_tests)")
    ap.add_argument("--valid", type=int, default=0, help="--from-stats: valid points per call (the kernel-only line's valid_points)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_points_bench.jsonl"))
    a = ap.parse_args()
    if a.from_stats:
        from_stats(a.from_stats, a.kernel_only or "A", a.tests, a.valid)
        return
    from lidar_object_detection_amd import _build
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    lines = [kernel_only(a.kernel_only, calib, a.calls)] if a.kernel_only else [
        r for b in a.batches.split(",") for r in end_to_end(b, calib, a.passes, a.warmup)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
