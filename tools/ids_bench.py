#!/usr/bin/env python3
"""One frame's masks into pipeline.run_frames, three forms of the SAME masks in one process, alternating repetition by repetition:
  (a) dense  uint8 host masks [M,H,W]                   (lpf_set_masks_u8 / lpf_run_wide with host masks: the parent's path, unchanged)
  (b) rle    rle.RleMasks of them                       (lpf_set_masks_rle / LPF_MASKS_RLE: the parent's path, unchanged)
  (c) ids    idmap.IdMasks: ONE uint16 map [H,W] + sel  (lpf_set_masks_ids / lpf_run_wide_ids)
The scan is sample frame 100 (109 355 host points, 25 boxes) with its 5 masks tiled (shifted copies) out to M = 5, 32, 64 and 256, as
tools/wide_rle_bench.py and DESIGN.md section 29 -- turned into a map: mask m gets ID 26001 + m, and where tiles overlap the LATER mask
owns the pixel.  The line says how many member pixels of the tiled masks that drops; all three forms are then the map's masks (the
dense form is IdMasks.to_dense(), the runs are made from it), so their results are compared on the first repetition.  After the warm-up
at least 50 repetitions of each form; per form the median, minimum and maximum in ms, and the bytes each form copies to the device
per call (dense: the masks; rle: runs + work units + run_off; ids: the map + sel).  One JSON line per M with the library's build id,
appended to --out.
  python tools/ids_bench.py [--masks 5,32,64,256] [--reps 50] [--warmup 5] [--out profiles/ids_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ids_bench.py --kernel-run --masks 32,256 [--reps 60]
  python tools/ids_bench.py --from-stats DIR
--kernel-run repeats the three forms without timing them; --from-stats turns that run's kernel statistics into the us of the decodes
(lpf_ids_*, lpf_rle_decode* and the fill in front of it), the packs and the erosion, one JSON line."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CHUNK = 1024                                                 # LPF_RLE_CHUNK: pixels per work unit
FORMS = ("dense", "rle", "ids")


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def same(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x["valid_indices"], y["valid_indices"]) and np.array_equal(x["count_mb"], y["count_mb"]), what
        assert np.array_equal(x["bg_assigned"], y["bg_assigned"]) and x["car_statistics"] == y["car_statistics"], what
        assert all(np.array_equal(p, q) for p, q in zip(x["car_point_sets"], y["car_point_sets"])), what


def forms_of(M, base):
    """(tiled uint8 [M,H,W], {form: masks}, encode ms of the runs)"""
    from lidar_object_detection_amd.idmap import IdMasks
    from lidar_object_detection_amd.rle import RleMasks
    tiled = np.ascontiguousarray(np.stack([np.roll(base[i % len(base)], 7 * (i // len(base)), axis=1) for i in range(M)]))
    ids = np.zeros(tiled.shape[1:], np.uint16)
    for m in range(M):
        ids[tiled[m] != 0] = 26001 + m                       # the later mask owns the pixel
    im = IdMasks(ids, 26001 + np.arange(M))
    dense = np.ascontiguousarray(im.to_dense())
    t0 = time.perf_counter()
    rle = RleMasks.from_dense(dense)
    return tiled, dict(dense=dense, rle=rle, ids=im), (time.perf_counter() - t0) * 1e3


def timed(M, g, base, calib, cam, boxes, reps, warmup):
    from lidar_object_detection_amd import pipeline
    tiled, masks, encode_ms = forms_of(M, base)
    T = calib["TrVeloToRect"]
    frames = {k: [pipeline.FrameInputs(100, g["points"], v, boxes)] for k, v in masks.items()}
    run = {k: (lambda k=k: pipeline.run_frames(frames[k], T, cam, 50.0, 10, True)) for k in FORMS}
    first = {k: run[k]() for k in FORMS}
    same(first["dense"], first["rle"], "rle")
    same(first["dense"], first["ids"], "ids")
    ts = {k: [] for k in FORMS}
    for r in range(warmup + reps):
        for form in FORMS[r % 3:] + FORMS[:r % 3]:
            t0 = time.perf_counter()
            run[form]()
            ts[form].append((time.perf_counter() - t0) * 1e3)
    rle, dense = masks["rle"], masks["dense"]
    n_runs = int(len(rle.runs))
    n_units = int(np.sum((rle.runs[:, 1].astype(np.int64) + CHUNK - 1) // CHUNK))
    line = dict(tool="ids_bench", M=M, F=1, W=dense.shape[2], H=dense.shape[1], points=int(len(g["points"])), boxes=len(boxes),
                member_pixels_tiled=int((tiled != 0).sum()), member_pixels_map=int(dense.sum()),
                member_pixels_dropped=int((tiled != 0).sum() - dense.sum()), runs=n_runs, work_units=n_units,
                encode_runs_from_dense_ms=round(encode_ms, 2),
                h2d_bytes=dict(dense=int(dense.nbytes), rle=8 * n_runs + 8 * n_units + 8 * (M + 1), ids=int(masks["ids"].ids.nbytes) + 4 * M))
    for form in FORMS:
        line[form] = spread(ts[form][warmup:])
    line["ids_over_dense_median"] = round(line["ids"]["ms_median"] / line["dense"]["ms_median"], 4)
    line["ids_over_rle_median"] = round(line["ids"]["ms_median"] / line["rle"]["ms_median"], 4)
    return line


def kernel_run(Ms, g, base, calib, cam, boxes, reps):
    """the run for rocprofv3: `reps` x the three forms, for every M"""
    from lidar_object_detection_amd import pipeline
    T = calib["TrVeloToRect"]
    for M in Ms:
        _, masks, _ = forms_of(M, base)
        for r in range(reps):
            for form in FORMS:
                pipeline.run_frames([pipeline.FrameInputs(100, g["points"], masks[form], boxes)], T, cam, 50.0, 10, True)
    pipeline.get_context(0).sync()


def from_stats(dirs):
    rows = {}
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        for r in (csv.DictReader(open(f[-1])) if f else ()):
            name = r["Name"]
            if any(k in name for k in ("lpf_ids_", "lpf_rle_decode", "lpf_pack", "lpf_wide_pack", "lpf_erode_packed", "fillBufferAligned")):
                rows[name.split("(")[0]] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                                                min_us=round(float(r["MinNs"]) / 1e3, 2), max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return dict(tool="ids_bench", kind="kernel_stats", kernels=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--masks", default="5,32,64,256")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ids_bench.jsonl"))
    a = ap.parse_args()
    from lidar_object_detection_amd import _build
    Ms = [int(x) for x in a.masks.split(",")]
    if a.from_stats:
        lines = [from_stats(a.from_stats)]
    else:
        from conftest import load_calib, load_golden, unpack_masks
        from lidar_object_detection_amd import kitti360
        calib = load_calib()
        cam = kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))
        g = load_golden(100)
        base = unpack_masks(g, "rect5", cam.height, cam.width).astype(np.uint8)
        boxes = [{"corners_velo": c.tolist()} for c in g["corners_velo"]]
        if a.kernel_run:
            kernel_run(Ms, g, base, calib, cam, boxes, a.reps)
            return
        lines = [timed(M, g, base, calib, cam, boxes, max(a.reps, 50), a.warmup) for M in Ms]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
