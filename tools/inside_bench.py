#!/usr/bin/env python3
"""V3's key set (corners_velo, inside_mask, car_points: V3:386-398) for a batch of real frames, two routes:
  (a) per-frame  run_frames, then pipeline.calculate_car_point_statistics(style 'v3') once per frame: one blocking lpf_points_in_boxes
                 call per frame that tests every car point against every box of the frame and brings the [B][sum k] matrix back -- the
                 only route to inside_mask before lpf_inside_masks.  Its statistics part is timed on one frame per distinct scan and
                 scaled to the batch (every 4th frame of the batch is the same scan), prints swallowed
  (b) batched    pipeline.car_statistics_v3_frames: the same pass plus ONE lpf_inside_masks call for the batch
  (c) kernel     --kernel-only: the pass once, then lpf_inside_masks alone on device-resident lists, for one
                 `rocprofv3 --kernel-trace --stats` run of its own; --from-stats DIR turns that run into the kernel's time, its bytes per
                 list entry (8 index + 16 point read, 1 + 8 + 12 written) and the GB/s that follow
Batch A: 146 frames, the four full-size golden frames (100, 1461, 2098, 2449: 16.9 M points) in turn, their five masks and their
visible boxes.  Batch B: the same frames with 256 detections each (a frame's five masks tiled).  One JSON line per (batch, route)
with the library's build id, appended to --out.
  python tools/inside_bench.py [--batches A,B] [--passes 7] [--out profiles/inside_masks_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/inside_bench.py --kernel-only A [--calls 20]
  python tools/inside_bench.py --from-stats DIR --kernel-only A [--calls 20]"""
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
BYTES_PER_ENTRY = 8 + 16 + 1 + 8 + 12


class Cam:
    def __init__(self, calib):
        self.K, self.width, self.height = np.asarray(calib["K"], np.float64)[:3, :3], int(calib["width"]), int(calib["height"])


def batch(which, calib, device_masks):
    """FrameInputs of batch A (five masks per frame) or B (256): the four scans in turn; masks on the GPU when device_masks"""
    from lidar_object_detection_amd import pipeline
    cam = Cam(calib)
    M = 5 if which == "A" else 256
    scans = []
    for name in NAMES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        m5 = np.unpackbits(g["masks_rect5_packed"], axis=-1)[..., :cam.width].astype(np.uint8)
        masks = np.ascontiguousarray(np.tile(m5, ((M + 4) // 5, 1, 1))[:M])
        if device_masks:
            import torch
            masks = torch.from_numpy(masks).cuda()
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        with contextlib.redirect_stdout(io.StringIO()):
            boxes = pipeline.prepare_boxes(raw, cam, calib["TrVeloToCam"], as_arrays=True)
        scans.append((np.ascontiguousarray(g["points"], dtype=np.float32), masks, boxes))
    colors = pipeline.default_colors(M)
    return [pipeline.FrameInputs(f, *scans[f % 4], colors) for f in range(FRAMES)], cam, M


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 2), ms_min=round(min(ts), 2), ms_max=round(max(ts), 2), passes=len(ts))


def end_to_end(which, calib, passes, warmup):
    from lidar_object_detection_amd import pipeline
    items, cam, M = batch(which, calib, device_masks=which == "B")
    T = np.asarray(calib["TrVeloToRect"])
    ctx = pipeline.get_context(0)

    def run_a():
        res = pipeline.run_frames(items, T, cam, 50.0, 10, True, ctx=ctx)
        return res, [r["car_point_sets"] for r in res]

    def stats_of(res, sets, f):
        with contextlib.redirect_stdout(io.StringIO()):
            return pipeline.calculate_car_point_statistics(sets[f], items[f].bboxes_3d, items[f].colors, 10, True, "v3")

    def run_b():
        return pipeline.car_statistics_v3_frames(items, T, cam, 50.0, 10, True, ctx=ctx)
    out = []
    ta, ts4, tb = [], [[] for _ in range(4)], []
    for p in range(warmup + passes):                         # the two routes in turn, pass by pass
        t0 = time.perf_counter()
        res, sets = run_a()
        t1 = time.perf_counter()
        per = []
        for f in range(4):                                   # the statistics of one frame per distinct scan
            t2 = time.perf_counter()
            st = stats_of(res, sets, f)
            per.append((time.perf_counter() - t2) * 1e3)
        t3 = time.perf_counter()
        got = run_b()
        t4 = time.perf_counter()
        if p == 0:                                           # the two routes agree (first frame of each scan)
            for f in range(4):
                want = stats_of(res, sets, f)
                assert len(want) == len(got[f]["car_statistics"])
                for x, y in zip(got[f]["car_statistics"], want):
                    assert x["matched_bbox_id"] == y["matched_bbox_id"] and x["points_inside_bbox"] == y["points_inside_bbox"]
                    assert (x["inside_mask"] is None) == (y["inside_mask"] is None)
                    assert x["inside_mask"] is None or np.array_equal(x["inside_mask"], y["inside_mask"])
        del st
        if p >= warmup:
            ta.append((t1 - t0) * 1e3)
            for f in range(4):
                ts4[f].append(per[f])
            tb.append((t4 - t3) * 1e3)
    entries = int(sum(int(r["inside_parts"]["off"][-1]) for r in got))
    cars = sum(len(r["car_statistics"]) for r in got)
    matched = sum(sum(1 for d in r["car_statistics"] if d["matched_bbox_id"] >= 0) for r in got)
    base = dict(batch=which, frames=FRAMES, masks_per_frame=M, list_entries=entries, cars_with_points=cars, matched_cars=matched,
                boxes_per_scan=[len(items[f].bboxes_3d) for f in range(4)])
    n_of = [sum(1 for f in range(FRAMES) if f % 4 == k) for k in range(4)]
    stats_scaled = [sum(n_of[k] * ts4[k][i] for k in range(4)) for i in range(passes)]
    total_a = [x + y for x, y in zip(ta, stats_scaled)]
    out.append(dict(route="a_per_frame", run_frames=spread(ta), statistics_scaled=spread(stats_scaled), total=spread(total_a),
                    statistics_ms_per_frame_by_scan=[round(statistics.median(t), 3) for t in ts4], **base))
    # (the two routes ran in turn: pass by pass the difference is taken on the same state of the host)
    out.append(dict(route="b_batched", total=spread(tb), beyond_run_frames_ms_median=round(statistics.median(tb) - statistics.median(ta), 2),
                    a_minus_b_pass_by_pass=spread([x - y for x, y in zip(total_a, tb)]), **base))
    return out


def kernel_only(which, calib, calls):
    """the pass once, then lpf_inside_masks `calls` times on device-resident points and lists (all five outputs)"""
    import torch
    from lidar_object_detection_amd import pipeline
    items, cam, M = batch(which, calib, device_masks=which == "B")
    ctx = pipeline.get_context(0)
    ctx.set_camera(np.asarray(calib["TrVeloToRect"]), cam.K, cam.width, cam.height, 0.0, 50.0)
    stacks, _, _ = pipeline._frame_mask_stacks(items, cam, ctx, 0, False)
    staged = ctx.stage_points([f.points for f in items])
    res, _ = pipeline._frames_pass(items, stacks, M, cam, True, 0, False, ctx, staged=staged)
    arrs = [torch.from_numpy(a).cuda() for a in pipeline.inside_list_arrays(res, M)]
    entries = int(arrs[1][:, M].sum())
    out = {k: torch.zeros(s, dtype=getattr(torch, ctx._INSIDE_OUT[k][0]), device="cuda")
           for k, s in (("inside", tuple(arrs[0].shape)), ("part_idx", tuple(arrs[0].shape)), ("part_xyz", tuple(arrs[0].shape) + (3,)),
                        ("n_inside", (FRAMES, M)), ("matched", (FRAMES, M)))}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        ctx.inside_masks(None, *arrs, min_points=10, out=out, staged=staged)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / calls
    return dict(route="c_kernel_only", batch=which, frames=FRAMES, masks_per_frame=M, list_entries=entries, inst_cap=int(arrs[0].shape[1]),
                longest_list=int(np.diff(arrs[1].cpu().numpy(), axis=1).max()), calls=calls, host_ms_per_call=round(ms, 3),
                bytes_per_entry=BYTES_PER_ENTRY, n_inside_total=int(out["n_inside"].sum()))


def from_stats(dirs, which, calls, entries):
    w = csv.writer(sys.stdout)
    w.writerow(["batch", "kernel", "calls", "avg_us", "min_us", "max_us", "list_entries", "bytes_per_entry", "GBps"])
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not f:
            continue
        for r in csv.DictReader(open(f[-1])):
            if "lpf_inside_cars" not in r["Name"]:
                continue
            avg = float(r["AverageNs"]) / 1e3
            w.writerow([which, r["Name"], r["Calls"], "%.2f" % avg, "%.2f" % (float(r["MinNs"]) / 1e3), "%.2f" % (float(r["MaxNs"]) / 1e3),
                        entries, BYTES_PER_ENTRY, "%.1f" % (entries * BYTES_PER_ENTRY / (avg * 1e-6) / 1e9) if entries else ""])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="A,B")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", metavar="BATCH")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--entries", type=int, default=0, help="--from-stats: list entries per call (the kernel-only line's list_entries)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inside_masks_bench.jsonl"))
    a = ap.parse_args()
    if a.from_stats:
        from_stats(a.from_stats, a.kernel_only or "A", a.calls, a.entries)
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
