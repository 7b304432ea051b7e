#!/usr/bin/env python3
"""secondtest.py's camera-view filter, V5's detailed box projection and secondtest's filter + transform + match for a batch of real
frames, two routes each, timed on the GPU machine's host:
  scalar   the package's scalar functions, one box (one frame) at a time: filter_bboxes_in_camera_view,
           project_3d_bbox_to_2d, and filter + transform_bboxes_to_velodyne + improved_match_detections_to_bboxes
  batched  filter_bboxes_in_camera_view_frames, project_3d_bboxes_to_2d_frames, secondtest_match_frames: ONE lpf_box_views call
           for the batch (and one lpf_match_2d call for the matcher)
and the native call alone (LpfContext.box_views on the batch's corners as one host array, and as one GPU tensor).
The batch: 146 frames that cycle the box sets of the four full-size golden frames (100, 1461, 2098, 2449: 31, 21, 186 and 314 boxes),
the detections of tests/golden/match2d_golden.npz.  Printed lines go to a buffer (both routes print the same ones).  Median of
--passes passes, the two routes of a row in turn; one JSON line per row with the library's build id, appended to --out.
  python tools/box_views_bench.py [--passes 20] [--out profiles/box_views_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/box_views_bench.py --kernel-only [--calls 20]
  python tools/box_views_bench.py --from-stats DIR"""
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
NAMES = ((100, "frame_0000000100"), (1461, "frame_0000001461_full"), (2098, "frame_0000002098_full"), (2449, "frame_0000002449_full"))
FRAMES = 146


class Cam:
    def __init__(self, calib):
        from lidar_object_detection_amd import kitti360
        self.K, self.width, self.height = np.asarray(calib["K"], np.float64), int(calib["width"]), int(calib["height"])
        self.cam2image = kitti360.CameraPerspective.cam2image.__get__(self)


def batch():
    """per frame: the raw box dicts (fresh ones), the detections and their colours"""
    from lidar_object_detection_amd import pipeline
    z = np.load(os.path.join(GOLDEN, "match2d_golden.npz"))
    scans = []
    for number, name in NAMES:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        dets = z["%d_dets" % number] if "%d_dets" % number in z.files else np.zeros((0, 4), np.float32)
        scans.append((raw, dets, pipeline.generate_consistent_colors(len(dets))))
    fresh = lambda: [[dict(b) for b in scans[f % 4][0]] for f in range(FRAMES)]
    return fresh, [scans[f % 4][1] for f in range(FRAMES)], [scans[f % 4][2] for f in range(FRAMES)], [len(s[0]) for s in scans]


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), passes=len(ts))


def timed(fn):
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        r = fn()
        return r, (time.perf_counter() - t0) * 1e3


def end_to_end(calib, passes, warmup):
    from lidar_object_detection_amd import pipeline
    cam = Cam(calib)
    fresh, dets, colors, per_scan = batch()
    Tvc = np.asarray(calib["TrVeloToCam"], np.float64)
    ctx = pipeline.get_context(0)

    def scalar_match(frames):
        out = []
        for f, boxes in enumerate(frames):
            kept, stats = pipeline.filter_bboxes_in_camera_view(boxes, cam)
            b3 = pipeline.transform_bboxes_to_velodyne(kept, Tvc)
            out.append((pipeline.improved_match_detections_to_bboxes(dets[f], b3, colors[f], cam), stats, b3))
        return out

    rows = {
        "filter": (lambda fr: [pipeline.filter_bboxes_in_camera_view(b, cam, False) for b in fr],
                   lambda fr: pipeline.filter_bboxes_in_camera_view_frames(fr, cam, False, ctx=ctx)),
        "filter_verbose": (lambda fr: [pipeline.filter_bboxes_in_camera_view(b, cam, True) for b in fr],
                           lambda fr: pipeline.filter_bboxes_in_camera_view_frames(fr, cam, True, ctx=ctx)),
        "project": (lambda fr: [[pipeline.project_3d_bbox_to_2d(b, cam) for b in boxes] for boxes in fr],
                    lambda fr: pipeline.project_3d_bboxes_to_2d_frames(fr, cam, ctx=ctx)),
        "secondtest_match": (scalar_match, lambda fr: pipeline.secondtest_match_frames(dets, fr, colors, cam, Tvc, ctx=ctx)),
    }
    base = dict(frames=FRAMES, boxes=sum(per_scan[f % 4] for f in range(FRAMES)), boxes_per_scan=per_scan)
    lines = []
    for name, (scalar, batched) in rows.items():
        ts, tb = [], []
        for p in range(warmup + passes):                     # the two routes in turn, pass by pass
            want, a = timed(lambda: scalar(fresh()))
            got, b = timed(lambda: batched(fresh()))
            if p == 0:                                       # the two routes agree
                assert repr(got) == repr(want), name
            if p >= warmup:
                ts.append(a)
                tb.append(b)
        copy_ms = statistics.median([timed(fresh)[1] for _ in range(5)])       # (both routes pay for the fresh dicts)
        lines.append(dict(row=name, scalar=spread(ts), batched=spread(tb), fresh_dicts_ms=round(copy_ms, 3),
                          ratio_of_medians=round(statistics.median(ts) / statistics.median(tb), 2),
                          scalar_minus_batched_pass_by_pass=spread([x - y for x, y in zip(ts, tb)]), **base))
    # the native call alone, and where the batched filter's time goes
    import torch
    frames = fresh()
    (slots, corners, off), t_gather = timed(lambda: pipeline._view_batch(frames))
    ctx.ensure_intrinsics(cam.K, cam.width, cam.height)
    dc = torch.from_numpy(corners).cuda()
    th, td, tg = [], [], []
    for p in range(warmup + passes):
        th.append(timed(lambda: ctx.box_views(corners, off, want=("keep", "reason")))[1])
        t0 = time.perf_counter()
        ctx.box_views(dc, off, want=("keep", "reason"))
        torch.cuda.synchronize()
        td.append((time.perf_counter() - t0) * 1e3)
        tg.append(timed(lambda: pipeline._view_batch(frames))[1])
    lines.append(dict(row="native_call", host_arrays=spread(th[warmup:]), device_tensors_synchronised=spread(td[warmup:]),
                      gather_corners_from_dicts=spread(tg[warmup:]), **base))
    return lines


def kernel_only(calib, calls):
    """lpf_box_views `calls` times on a device-resident batch, every output asked for"""
    import torch
    from lidar_object_detection_amd import pipeline
    from lidar_object_detection_amd._native import LpfContext
    cam = Cam(calib)
    fresh, _, _, per_scan = batch()
    _, corners, off = pipeline._view_batch(fresh())
    ctx = pipeline.get_context(0)
    ctx.ensure_intrinsics(cam.K, cam.width, cam.height)
    dc = torch.from_numpy(corners).cuda()
    Tcv = np.linalg.inv(np.asarray(calib["TrVeloToCam"], np.float64))
    ctx.box_views(dc, off, T_cam_to_velo=Tcv, want=LpfContext.BOX_VIEWS_WANT)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        res = ctx.box_views(dc, off, T_cam_to_velo=Tcv, want=LpfContext.BOX_VIEWS_WANT)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / calls
    return dict(row="kernel_only", frames=FRAMES, boxes=len(corners), boxes_per_scan=per_scan, calls=calls, host_ms_per_call=round(ms, 3),
                kept=int(res["keep"].sum()), bytes_per_box=192 + 293)


def from_stats(dirs):
    w = csv.writer(sys.stdout)
    w.writerow(["kernel", "calls", "avg_us", "min_us", "max_us"])
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not f:
            continue
        for r in csv.DictReader(open(f[-1])):
            if "lpf_box_views_kernel" in r["Name"]:
                w.writerow([r["Name"], r["Calls"], "%.2f" % (float(r["AverageNs"]) / 1e3), "%.2f" % (float(r["MinNs"]) / 1e3),
                            "%.2f" % (float(r["MaxNs"]) / 1e3)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_views_bench.jsonl"))
    a = ap.parse_args()
    if a.from_stats:
        from_stats(a.from_stats)
        return
    from lidar_object_detection_amd import _build
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    lines = [kernel_only(calib, a.calls)] if a.kernel_only else end_to_end(calib, a.passes, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
