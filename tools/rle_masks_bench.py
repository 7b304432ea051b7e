#!/usr/bin/env python3
"""Host masks into the library, two forms of the same masks in one process, alternating repetition by repetition:
  (a) dense  LpfContext.set_masks(uint8 host [F,M,H,W]) + run_batch     (lpf_set_masks_u8, on_device = 0)
  (b) rle    LpfContext.set_masks_rle([RleMasks] * F) + run_batch       (lpf_set_masks_rle: the runs are decoded on the GPU)
Synthetic scenes (synthetic.py) at 1408 x 376, 120 000 points per frame already on the GPU (so that only the masks cross the bus in the
timed part); mask m of a frame is a disk (even m) or the rectangle of a projected 3-D box (odd m).  M = 5 and 32, F = 1 and 20.  After
the warm-up at least 50 repetitions of each form; per form the median, minimum and maximum of set + run in ms, of the set call alone and
of the run alone, and the bytes each form copies to the device per call (dense: the masks; rle: runs + work units + run_off).  The two
forms' label images and run results are compared on the first repetition.  One JSON line per (M, F) with the library's build id,
appended to --out.
  python tools/rle_masks_bench.py [--reps 50] [--warmup 5] [--out profiles/rle_masks_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rle_masks_bench.py --kernel-run M,F [--reps 60]
  python tools/rle_masks_bench.py --from-stats DIR --kernel-run M,F
--kernel-run repeats three forms: dense host masks (sparse frames: no pack is launched, the tiles read the staged masks, LpfDirect), the
runs (fill + lpf_rle_decode, then packed tiles), and the dense masks as a GPU tensor packed at the call (lpf_pack16, then packed tiles);
--from-stats turns that run into the us of the decode, pack, erosion and tile kernels and of the fill, one JSON line."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ((5, 1), (32, 1), (5, 20), (32, 20))
POINTS = 120_000
CHUNK = 1024                                                 # LPF_RLE_CHUNK: pixels per work unit


def scene_masks(M, seed, calib):
    """(points f32 [n,4], masks uint8 [M,H,W], corners_velo) of one synthetic frame: disks and projected-box rectangles"""
    from lidar_object_detection_amd import synthetic as S
    _, _, K, W, H = S.default_calibration(calib)
    sc = S.scene(POINTS, n_masks=M, n_boxes=max(M, 16), seed=seed, calib=calib)
    masks = sc["masks"].copy()
    for m in range(1, M, 2):
        c = sc["corners_cam0"][m]
        z = np.maximum(c[:, 2], 0.1)
        u, v = K[0, 0] * c[:, 0] / z + K[0, 2], K[1, 1] * c[:, 1] / z + K[1, 2]
        x0, x1 = int(np.clip(u.min(), 0, W - 1)), int(np.clip(u.max(), 0, W - 1))
        y0, y1 = int(np.clip(v.min(), 0, H - 1)), int(np.clip(v.max(), 0, H - 1))
        masks[m] = 0
        masks[m, y0:y1 + 1, x0:x1 + 1] = 1
    return sc["points"], masks, sc["corners_velo"][:16]


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def setup(M, F, calib):
    import torch
    from lidar_object_detection_amd import synthetic as S
    from lidar_object_detection_amd._native import LpfContext
    from lidar_object_detection_amd.rle import RleMasks
    _, T, K, W, H = S.default_calibration(calib)
    frames = [scene_masks(M, 7000 + 31 * f + M, calib) for f in range(F)]
    dense = np.ascontiguousarray(np.stack([m for _, m, _ in frames]))
    t0 = time.perf_counter()
    rles = [RleMasks.from_dense(m) for m in dense]
    encode_ms = (time.perf_counter() - t0) * 1e3
    ctx = LpfContext(0)
    ctx.set_camera(T, K, W, H, 0.0, 50.0)
    ctx.set_boxes([b for _, _, b in frames])
    pts = [torch.from_numpy(p).cuda() for p, _, _ in frames]
    torch.cuda.synchronize()
    return ctx, dense, rles, pts, encode_ms


def one(ctx, form, dense, rles, pts):
    t0 = time.perf_counter()
    if form == "dense":
        ctx.set_masks(dense)
    else:
        ctx.set_masks_rle(rles)
    t1 = time.perf_counter()
    res = ctx.run_batch(pts, want_uv=False, want_label=False, want_valid_uv=True, pinned=True)
    t2 = time.perf_counter()
    return res, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def timed(M, F, calib, reps, warmup):
    ctx, dense, rles, pts, encode_ms = setup(M, F, calib)
    ctx.set_masks(dense)
    img = ctx.get_label_image()
    ctx.set_masks_rle(rles)
    assert np.array_equal(ctx.get_label_image(), img)        # the two forms are the same masks
    ts = {"dense": [], "rle": []}
    for r in range(warmup + reps):
        keep = {}
        for form in ("dense", "rle") if r % 2 == 0 else ("rle", "dense"):
            res, t_set, t_run = one(ctx, form, dense, rles, pts)
            ts[form].append((t_set + t_run, t_set, t_run))
            if r == 0:
                keep[form] = [(x["n_valid"], x["inst_count"].copy(), x["count_mb"].copy(), x["label_valid"].copy()) for x in res]
        if r == 0:
            for a, b in zip(keep["dense"], keep["rle"]):
                assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    n_runs = int(sum(len(x.runs) for x in rles))
    n_units = int(sum(int(np.sum((x.runs[:, 1].astype(np.int64) + CHUNK - 1) // CHUNK)) for x in rles))
    line = dict(tool="rle_masks_bench", M=M, F=F, W=dense.shape[3], H=dense.shape[2], points_per_frame=POINTS, runs=n_runs, work_units=n_units,
                member_fraction=round(float(dense.mean()), 4), encode_from_dense_ms=round(encode_ms, 2),
                h2d_bytes=dict(dense=int(dense.nbytes), rle=8 * n_runs + 8 * n_units + 8 * (F * M + 1)))
    for form in ("dense", "rle"):
        t = ts[form][warmup:]
        line[form] = dict(set_plus_run=spread([x[0] for x in t]), set=spread([x[1] for x in t]), run=spread([x[2] for x in t]))
    line["rle_over_dense_median"] = round(line["rle"]["set_plus_run"]["ms_median"] / line["dense"]["set_plus_run"]["ms_median"], 4)
    ctx.close()
    return line


def kernel_run(M, F, calib, reps):
    """the run for rocprofv3: `reps` x (dense host masks, runs, and the same masks as a GPU tensor that is not lent -- the form that is
    packed at the call (lpf_pack16), which sparse frames of host masks are not: their tiles read the staged masks directly)"""
    import torch
    ctx, dense, rles, pts, _ = setup(M, F, calib)
    on_gpu = torch.from_numpy(dense).cuda()
    torch.cuda.synchronize()
    for r in range(reps):
        for form in ("dense", "rle"):
            one(ctx, form, dense, rles, pts)
        one(ctx, "dense", on_gpu, rles, pts)
    ctx.sync()
    ctx.close()


def from_stats(dirs, M, F):
    rows = {}
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        for r in (csv.DictReader(open(f[-1])) if f else ()):
            name = r["Name"]
            if any(k in name for k in ("lpf_rle_decode", "lpf_pack", "lpf_erode_packed", "lpf_k1_project_t", "fillBufferAligned")):
                rows[name.split("(")[0]] = dict(calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                                                min_us=round(float(r["MinNs"]) / 1e3, 2), max_us=round(float(r["MaxNs"]) / 1e3, 2))
    return dict(tool="rle_masks_bench", kind="kernel_stats", M=M, F=F, kernels=rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-run", metavar="M,F")
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_masks_bench.jsonl"))
    a = ap.parse_args()
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    case = tuple(int(v) for v in a.kernel_run.split(",")) if a.kernel_run else None
    if case and not a.from_stats:
        kernel_run(case[0], case[1], calib, a.reps)
        return
    from lidar_object_detection_amd import _build
    lines = [from_stats(a.from_stats, *(case or (0, 0)))] if a.from_stats else [timed(M, F, calib, max(a.reps, 50), a.warmup) for M, F in CASES]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
