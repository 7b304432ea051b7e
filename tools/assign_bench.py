#!/usr/bin/env python3
"""V5's matcher for a batch of frames (improved_match_detections_to_bboxes, V5:307-416), the assignment on the host or on the GPU:
  host     pipeline.improved_match_detections_frames(assign="host"): one lpf_match_2d call, the five [D,B] matrices downloaded, scipy's
           linear_sum_assignment once per frame
  device   the same function with assign="device": one lpf_assign_2d call (pair scores, SciPy's assignment and the thresholds on the
           GPU), a few words per detection downloaded
The two alternate in one process, pass by pass, prints swallowed; the median, the minimum and the maximum of --passes passes each.  Also the raw
LpfContext.assign_2d call on GPU tensors, timed to completion.  Workload: tools/match2d_bench.py's -- the boxes of
the four full-size golden frames in turn to 146 frames with 5, 32 and 256 seeded float32 detections per frame -- and one frame alone
(256 detections against the 314-box frame).  Appends one JSON line per (frames, detections) with the library's build id.
  python tools/assign_bench.py [--dets 5,32,256] [--passes 20] [--out profiles/assign_bench.jsonl]
  python tools/assign_bench.py --kernel-run     five raw calls of the 146 x 256 batch and nothing else: the run to put under
                                                `rocprofv3 --kernel-trace --stats` for the durations of lpf_as_pack / lpf_as_solve"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match2d_bench as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", default="5,32,256")
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assign_bench.jsonl"))
    a = ap.parse_args()
    import torch
    from lidar_object_detection_amd import _build, pipeline
    calib = dict(np.load(os.path.join(M.GOLDEN, "calib_cam0.npz")))
    cam = M.Cam(calib)
    ctx = pipeline.get_context(0)
    sets = []
    for name in M.BOX_FILES:
        g = np.load(os.path.join(M.GOLDEN, name + ".npz"))
        raw = [{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])]
        boxes = list(pipeline.prepare_boxes(raw, cam, calib["TrVeloToCam"], keep_all=True))
        bb = np.array([b["_bbox2d"] if b["_bbox2d"] is not None else [0.0] * 4 for b in boxes], np.float64)
        front = np.array([b["_front"] for b in boxes], np.int32)
        sets.append((boxes, bb, front))

    def workload(frames, D):
        which = [f % len(sets) for f in range(frames)] if frames > 1 else [len(sets) - 1]
        dets = [M.detections(9000 + f, D, sets[k][1], sets[k][2], cam.width, cam.height) for f, k in enumerate(which)]
        return dets, [sets[k][0] for k in which], [sets[k][1] for k in which], [sets[k][2] for k in which]

    def to_gpu(*lists):
        return [[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrs] for arrs in lists]

    if a.kernel_run:
        dets, _, bbs, fronts = workload(M.FRAMES, 256)
        dev = to_gpu(dets, bbs, fronts)
        for _ in range(5):
            ctx.assign_2d(*dev)
            torch.cuda.synchronize()
        return

    lines = []
    for frames, D in [(M.FRAMES, int(x)) for x in a.dets.split(",")] + [(1, 256)]:
        dets, boxes, bbs, fronts = workload(frames, D)
        colors = [pipeline.generate_consistent_colors(D)] * frames
        routes = {"host": [], "device": []}
        texts = {}
        for p in range(a.warmup + a.passes):
            for route in ("host", "device"):
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    t0 = time.perf_counter()
                    out = pipeline.improved_match_detections_frames(dets, boxes, colors, cam, ctx=ctx, assign=route)
                    ms = (time.perf_counter() - t0) * 1e3
                if p >= a.warmup:
                    routes[route].append(ms)
                texts[route] = (buf.getvalue(), [len(o) for o in out])
        assert texts["host"] == texts["device"]             # the same lines and lists
        dev = to_gpu(dets, bbs, fronts)
        raw = []
        for p in range(a.warmup + a.passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.assign_2d(*dev)
            torch.cuda.synchronize()
            if p >= a.warmup:
                raw.append((time.perf_counter() - t0) * 1e3)
        kw = dict(frames=frames, dets_per_frame=D, pairs=sum(len(d) * len(b) for d, b in zip(dets, bbs)), passes=a.passes,
                  host_ms_median=round(statistics.median(routes["host"]), 3), host_ms_min=round(min(routes["host"]), 3), host_ms_max=round(max(routes["host"]), 3),
                  device_ms_median=round(statistics.median(routes["device"]), 3), device_ms_min=round(min(routes["device"]), 3),
                  device_ms_max=round(max(routes["device"]), 3),
                  raw_assign_2d_ms_median=round(statistics.median(raw), 3), raw_assign_2d_ms_min=round(min(raw), 3), raw_assign_2d_ms_max=round(max(raw), 3),
                  source_id=_build.library_id(_build.LIB))
        lines.append(kw)
        print(json.dumps(kw), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for kw in lines:
            f.write(json.dumps(kw) + "\n")


if __name__ == "__main__":
    main()
