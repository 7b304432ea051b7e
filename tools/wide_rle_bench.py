#!/usr/bin/env python3
"""Host masks into the wide pass, two forms of the same masks in one process, alternating repetition by repetition:
  (a) dense  LpfContext.run_wide(points, uint8 host [1,M,H,W])      (lpf_wide_input.f32 = LPF_MASKS_U8, on_device = 0)
  (b) rle    LpfContext.run_wide(points, RleMasks)                   (LPF_MASKS_RLE: the runs are decoded into the planes on the GPU)
and pipeline.run_frames on the same RleMasks frame, per group of 32 masks (set_masks_rle + a narrow run per group: what run_frames did
for such frames before the wide pass took runs) against the one wide pass it makes now.  The scan is sample frame 100 (109 355 points,
25 boxes) with its 5 masks tiled (shifted copies) out to M = 40, 64, 128 and 256 masks, as tools/wide_masks_bench.py and DESIGN.md
section 12.  After the warm-up at least 50 repetitions of each; per form the median, minimum and maximum in ms, and the bytes each form
copies to the device per call (dense: the masks; rle: runs + work units + run_off).  The two forms' results are compared on the first
repetition.  One JSON line per M with the library's build id, appended to --out.
  python tools/wide_rle_bench.py [--masks 40,64,128,256] [--reps 50] [--warmup 5] [--out profiles/wide_rle_bench.jsonl]"""
import argparse
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


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def same(a, b):
    for x, y in zip(a, b):
        assert x["n_valid"] == y["n_valid"] and np.array_equal(x["inst_count"], y["inst_count"]) and np.array_equal(x["count_mb"], y["count_mb"])
        assert np.array_equal(x["label_valid_words"], y["label_valid_words"]) and np.array_equal(x["valid_idx"], y["valid_idx"])


def timed(M, g, base, calib, cam, boxes, reps, warmup):
    from lidar_object_detection_amd import pipeline
    from lidar_object_detection_amd._native import LPF_MAX_MASKS
    from lidar_object_detection_amd.rle import RleMasks
    dense = np.ascontiguousarray(np.stack([np.roll(base[i % len(base)], 7 * (i // len(base)), axis=1) for i in range(M)]))
    t0 = time.perf_counter()
    rle = RleMasks.from_dense(dense)
    encode_ms = (time.perf_counter() - t0) * 1e3
    ctx = pipeline.get_context(0)
    T = calib["TrVeloToRect"]
    pts = [g["points"]]
    want = dict(want_uv=False, want_valid_uv=True)
    frames = [pipeline.FrameInputs(100, g["points"], rle, boxes)]

    def wide():
        return pipeline.run_frames(frames, T, cam, 50.0, 10, True)

    def grouped():
        ctx.set_erosion_element(3)
        ctx.set_camera(T, cam.K, cam.width, cam.height, 0.0, 50.0)
        return pipeline._run_frames_in_mask_groups(frames, [rle], T, cam, 50.0, 10, True, 0, False, 0, ctx, group=LPF_MAX_MASKS)

    first = wide()                                           # (sets the camera and the frame's boxes: every group sets the same ones again)
    again = grouped()
    assert np.array_equal(first[0]["count_mb"], again[0]["count_mb"]) and np.array_equal(first[0]["valid_indices"], again[0]["valid_indices"])
    forms = {"dense": lambda: ctx.run_wide(pts, dense[None], **want), "rle": lambda: ctx.run_wide(pts, rle, **want),
             "run_frames_wide": wide, "run_frames_groups": grouped}
    same(forms["dense"](), forms["rle"]())
    ts = {k: [] for k in forms}
    for r in range(warmup + reps):
        for pair in (("dense", "rle"), ("run_frames_wide", "run_frames_groups")):
            for form in pair if r % 2 == 0 else pair[::-1]:
                t0 = time.perf_counter()
                forms[form]()
                ts[form].append((time.perf_counter() - t0) * 1e3)
    n_runs = int(len(rle.runs))
    n_units = int(np.sum((rle.runs[:, 1].astype(np.int64) + CHUNK - 1) // CHUNK))
    line = dict(tool="wide_rle_bench", M=M, F=1, W=dense.shape[2], H=dense.shape[1], points=int(len(g["points"])), boxes=len(boxes),
                runs=n_runs, work_units=n_units, member_fraction=round(float(dense.mean()), 4), encode_from_dense_ms=round(encode_ms, 2),
                h2d_bytes=dict(dense=int(dense.nbytes), rle=8 * n_runs + 8 * n_units + 8 * (M + 1)))
    for form in forms:
        line[form] = spread(ts[form][warmup:])
    line["rle_over_dense_median"] = round(line["rle"]["ms_median"] / line["dense"]["ms_median"], 4)
    line["wide_over_groups_median"] = round(line["run_frames_wide"]["ms_median"] / line["run_frames_groups"]["ms_median"], 4)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--masks", default="40,64,128,256")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_rle_bench.jsonl"))
    a = ap.parse_args()
    from conftest import load_calib, load_golden, unpack_masks
    from lidar_object_detection_amd import _build, kitti360
    calib = load_calib()
    cam = kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))
    g = load_golden(100)
    base = unpack_masks(g, "rect5", cam.height, cam.width).astype(np.uint8)
    boxes = [{"corners_velo": c.tolist()} for c in g["corners_velo"]]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for M in [int(x) for x in a.masks.split(",")]:
            r = timed(M, g, base, calib, cam, boxes, max(a.reps, 50), a.warmup)
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
