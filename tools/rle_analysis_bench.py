#!/usr/bin/env python3
"""Host masks into the two analysis calls, two forms of the same masks in one process, alternating repetition by repetition:
  (a) dense  pipeline.depth_maps_frames / first_match_frames on uint8 host masks      (lpf_depth_maps / lpf_first_match: the parent's path)
  (b) rle    the same functions on rle.RleMasks frames                                (lpf_depth_maps_rle / lpf_first_match_rle)
Workloads: DESIGN section 16's -- the 4 full-size frames with frame 100's five masks tiled to M = 5 / 40 / 256 (depth_maps_bench.py's
tiledM) -- and section 24's full4x5 / full4x40 / full4x256 (first_match_bench.py's).  After the warm-up at least 50 repetitions of each
form; per form the median, minimum and maximum in ms, the bytes each form copies to the device per call (dense: the masks; rle: runs
+ work units + run_off of the batch), and RleMasks.from_dense's time on its own (it is not part of either form's time).  The two forms'
results are compared on the first repetition.  One JSON line per (call, M) with the library's build id, appended to --out.
  python tools/rle_analysis_bench.py [--calls depth_maps,first_match] [--masks 5,40,256] [--reps 50] [--warmup 5] [--out profiles/rle_analysis_bench.jsonl]
For the kernels alone, one run of its own under the profiler (no counters in it):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rle_analysis_bench.py --kernel-run [--kcalls 10]
lpf_first_match on device-resident uint8 masks, then lpf_first_match_rle on the same masks as runs (device points, colours and
outputs), kcalls each, at M = 5, 40, 256 in that order; --from-trace DIR cuts the kernel trace at the calls' ends (every call ends with
lpf_fm_scatter) and prints one CSV row per (M, form, kernel): the count kernels, the scan and scatter, the decode and the fill kernels
that zero the planes and counters."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CHUNK = 1024                                                 # LPF_RLE_CHUNK: pixels per work unit
DMAX = 30.0
KERNEL_MS = (5, 40, 256)


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), reps=len(ts))


def rle_bytes(rles, M):
    runs = sum(len(r.runs) for r in rles)
    units = sum(int(np.sum((r.runs[:, 1].astype(np.int64) + CHUNK - 1) // CHUNK)) for r in rles)
    return 8 * runs + 8 * units + 8 * (len(rles) * M + 1), runs, units


def same_depth_maps(a, b):
    for fa, fb in zip(a, b):
        assert len(fa) == len(fb)
        for (ia, x), (ib, y) in zip(fa, fb):
            assert ia == ib and np.array_equal(x.pixels, y.pixels) and np.array_equal(x.depth, y.depth) and np.array_equal(x.point_idx, y.point_idx)


def same_first_match(a, b):
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k], y[k]), k


def timed(call, M, calib, reps, warmup):
    import depth_maps_bench as DM
    import first_match_bench as FM
    from lidar_object_detection_amd import pipeline
    from lidar_object_detection_amd.rle import RleMasks
    cam, T = FM.Cam(calib), np.asarray(calib["TrVeloToRect"])
    data = DM.case_frames("tiled%d" % M, cam.width, cam.height) if call == "depth_maps" else FM.frames_of("full4x%d" % M, calib)
    t0 = time.perf_counter()
    rles = [RleMasks.from_dense(m) for _, m in data]
    encode_ms = (time.perf_counter() - t0) * 1e3
    cols = pipeline.default_colors(M)
    dense = [pipeline.FrameInputs(i, p, m, colors=cols) for i, (p, m) in enumerate(data)]
    runs = [pipeline.FrameInputs(i, p, r, colors=cols) for i, ((p, _), r) in enumerate(zip(data, rles))]
    ctx = pipeline.get_context(0)
    fn = pipeline.depth_maps_frames if call == "depth_maps" else pipeline.first_match_frames
    forms = {"dense": lambda: fn(dense, T, cam, DMAX, ctx=ctx), "rle": lambda: fn(runs, T, cam, DMAX, ctx=ctx)}
    (same_depth_maps if call == "depth_maps" else same_first_match)(forms["dense"](), forms["rle"]())
    ts = {k: [] for k in forms}
    for r in range(warmup + reps):
        for form in ("dense", "rle") if r % 2 == 0 else ("rle", "dense"):
            t0 = time.perf_counter()
            forms[form]()
            ts[form].append((time.perf_counter() - t0) * 1e3)
    b_rle, n_runs, n_units = rle_bytes(rles, M)
    line = dict(tool="rle_analysis_bench", call=call, M=M, F=len(data), W=cam.width, H=cam.height, points=int(sum(len(p) for p, _ in data)),
                runs=n_runs, work_units=n_units, member_fraction=round(float(np.mean([m.mean() for _, m in data])), 4),
                from_dense_ms=round(encode_ms, 2), h2d_mask_bytes=dict(dense=int(sum(m.nbytes for _, m in data)), rle=b_rle))
    for form in forms:
        line[form] = spread(ts[form][warmup:])
    line["rle_over_dense_median"] = round(line["rle"]["ms_median"] / line["dense"]["ms_median"], 4)
    line["verdict"] = "rle wins" if line["rle_over_dense_median"] < 1 else "rle LOSES"
    return line


def kernel_run(calib, kcalls):
    """the two native calls alone, kcalls each per M, on device-resident points, colours and outputs (every output)"""
    import torch
    import first_match_bench as FM
    from lidar_object_detection_amd import pipeline
    from lidar_object_detection_amd.rle import RleMasks
    cam = FM.Cam(calib)
    ctx = pipeline.get_context(0)
    ctx.set_camera(np.asarray(calib["TrVeloToRect"]), cam.K, cam.width, cam.height, 0.0, DMAX)
    lines = []
    for M in KERNEL_MS:
        data = FM.frames_of("full4x%d" % M, calib)
        batch = torch.from_numpy(np.stack([m for _, m in data])).cuda()
        rles = [RleMasks.from_dense(m) for _, m in data]
        colors = torch.rand((len(data), M, 3), dtype=torch.float64, device="cuda")
        staged = ctx.stage_points([p for p, _ in data])
        outs = {}
        for form, masks in (("dense_device", batch), ("rle", rles)):
            out = None
            for _ in range(kcalls):
                out = ctx.first_match(None, masks, colors, out=out and {k: v for k, v in out.items() if k != "frame_off"}, staged=staged)
                torch.cuda.synchronize()
            outs[form] = out
        for k in outs["rle"]:
            if k != "frame_off":
                assert torch.equal(outs["rle"][k], outs["dense_device"][k]), k
        lines.append(dict(tool="rle_analysis_bench", route="kernel_run", M=M, frames=len(data), points=int(staged[0][-1]), calls_per_form=kcalls,
                          car_points=int(outs["rle"]["n_car"].sum()), background_points=int(outs["rle"]["n_bg"].sum())))
    return lines


def from_trace(dirs, kcalls):
    w = csv.writer(sys.stdout)
    w.writerow(["M", "form", "kernel", "dispatches", "per_call", "avg_us", "min_us", "max_us", "us_per_call"])
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
        if not f:
            continue
        rows = sorted(csv.DictReader(open(f[-1])), key=lambda r: int(r["Start_Timestamp"]))
        done, started, phase = 0, False, {}
        for r in rows:
            name = r["Kernel_Name"]
            if not started:                                  # (what the staging of points and masks launched before the first call)
                if "lpf_" not in name:
                    continue
                started = True
            p = done // kcalls
            if p >= 2 * len(KERNEL_MS):
                break
            short = name.split("(")[0].replace("void ", "")
            if "lpf_" not in short:
                short = "fill / copy kernel (" + short[:40] + ")"
            phase.setdefault((p, short), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            if "lpf_fm_scatter" in name:
                done += 1
        for (p, short), us in sorted(phase.items()):
            w.writerow([KERNEL_MS[p // 2], ("dense_device", "rle")[p % 2], short, len(us), "%.1f" % (len(us) / kcalls), "%.2f" % statistics.mean(us),
                        "%.2f" % min(us), "%.2f" % max(us), "%.2f" % (sum(us) / kcalls)])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", default="depth_maps,first_match")
    ap.add_argument("--masks", default="5,40,256")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-run", action="store_true")
    ap.add_argument("--kcalls", type=int, default=10)
    ap.add_argument("--from-trace", nargs="+", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_analysis_bench.jsonl"))
    a = ap.parse_args()
    if a.from_trace:
        from_trace(a.from_trace, a.kcalls)
        return
    from lidar_object_detection_amd import _build
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        lines = kernel_run(calib, a.kcalls) if a.kernel_run else (
            timed(c, int(M), calib, max(a.reps, 50), a.warmup) for c in a.calls.split(",") for M in a.masks.split(","))
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
