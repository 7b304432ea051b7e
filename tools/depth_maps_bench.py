#!/usr/bin/env python3
"""Per-car depth maps (seg_with_pointcloud.py:160-170) of a batch of frames, two routes:
  batched    pipeline.depth_maps_frames: ONE lpf_depth_maps call for the batch, sparse lists back, one host wait
  per_frame  pipeline.per_car_depth_maps once per frame: lpf_depth_image copies the dense f64 image back, NumPy builds M dense maps
Cases (host scans and host uint8 masks, as a frame loop holds them after np.fromfile and the segmenter's .cpu()):
  golden23   the 20 sample frames + the 3 full-size frames with their rect5 masks (0 to 5 per frame)
  tiledM     the 4 full-size frames (100, 1461, 2098, 2449) with frame 100's five masks tiled out to M (5, 40, 256)
Prints one JSON line per (route, case): the median host wall time of the whole batch over the passes.
  python tools/depth_maps_bench.py [--routes batched,per_frame] [--cases golden23,tiled5,tiled40,tiled256] [--passes 20]
Under `rocprofv3 --kernel-trace --stats` run one (route, case) per process (--routes R --cases C --passes 5 --warmup 2) into a directory
named <route>_<case>; --from-stats DIR... turns such runs into per-kernel microseconds per batch, one CSV row per (route, case, kernel)."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL = ("frame_0000000100.npz", "frame_0000001461_full.npz", "frame_0000002098_full.npz", "frame_0000002449_full.npz")


class Cam:
    def __init__(self, calib):
        self.width, self.height, self.K = int(calib["width"]), int(calib["height"]), np.asarray(calib["K"])[:3, :3]


def _masks(g, W):
    if "masks_rect5_packed" not in g.files:
        return None
    return np.unpackbits(g["masks_rect5_packed"], axis=-1)[..., :W].astype(np.uint8)


def case_frames(case, W, H):
    """[(points f32 [N,4], masks uint8 [M,H,W])] of a case"""
    if case == "golden23":
        idx = json.load(open(os.path.join(GOLDEN, "index.json")))
        names = ["frame_%010d.npz" % r["frame"] for r in idx["frames"]] + ["frame_%010d_full.npz" % r["frame"] for r in idx["full_frames"]]
        out = []
        for n in names:
            g = np.load(os.path.join(GOLDEN, n))
            m = _masks(g, W)
            out.append((np.ascontiguousarray(g["points"], np.float32), m if m is not None else np.zeros((0, H, W), np.uint8)))
        return out
    M = int(case[len("tiled"):])
    m5 = _masks(np.load(os.path.join(GOLDEN, FULL[0])), W)
    masks = np.ascontiguousarray(np.stack([np.roll(m5[i % 5], 37 * (i // 5), axis=1) for i in range(M)]))
    return [(np.ascontiguousarray(np.load(os.path.join(GOLDEN, n))["points"], np.float32), masks) for n in FULL]


def measure(route, case, calib, passes, warmup):
    from lidar_object_detection_amd import pipeline
    cam = Cam(calib)
    T = np.asarray(calib["TrVeloToRect"])
    frames = case_frames(case, cam.width, cam.height)
    ctx = pipeline.get_context(0)
    if route == "batched":
        inputs = [pipeline.FrameInputs(i, p, m) for i, (p, m) in enumerate(frames)]

        def run():
            return pipeline.depth_maps_frames(inputs, T, cam, 30.0, ctx=ctx)
    else:
        def run():
            return [pipeline.per_car_depth_maps(p, T, cam, m, 30.0) for p, m in frames]
    for _ in range(warmup):
        run()
    ctx.stats(reset=True)
    t = []
    for _ in range(passes):
        t0 = time.perf_counter()
        run()
        t.append(time.perf_counter() - t0)
    st = ctx.stats()
    med = statistics.median(t) * 1e3
    return dict(route=route, case=case, frames=len(frames), max_masks=max(int(m.shape[0]) for _, m in frames),
                cars=int(sum(m.shape[0] for _, m in frames)), passes=passes,
                ms_per_batch_median=round(med, 3), ms_per_batch_min=round(min(t) * 1e3, 3), us_per_frame_median=round(med * 1e3 / len(frames), 1),
                host_waits_per_batch=st["host_waits"] / passes)


def from_stats(dirs, calls):
    import csv
    w = csv.writer(sys.stdout)
    w.writerow(["route", "case", "kernel", "calls", "us_per_batch"])
    for d in dirs:
        base = os.path.basename(d.rstrip("/"))
        route = "per_frame" if base.startswith("per_frame_") else "batched"
        case = base[len(route) + 1:]
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not f:
            continue
        tot = 0.0
        for r in csv.DictReader(open(f[-1])):
            if not r["Name"].startswith(("lpf_", "void lpf_")):
                continue
            us = int(r["TotalDurationNs"]) / 1e3 / calls
            tot += us
            w.writerow([route, case, r["Name"].split("(")[0].replace("void ", ""), r["Calls"], "%.2f" % us])
        w.writerow([route, case, "TOTAL lpf_*", "", "%.2f" % tot])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--routes", default="batched,per_frame")
    ap.add_argument("--cases", default="golden23,tiled5,tiled40,tiled256")
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    a = ap.parse_args()
    if a.from_stats:
        from_stats(a.from_stats, a.passes + a.warmup)
        return
    from lidar_object_detection_amd import _build
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    sid = _build.source_id()
    for case in a.cases.split(","):
        for route in a.routes.split(","):
            r = measure(route, case, calib, a.passes, a.warmup)
            r["source_id"] = sid
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
