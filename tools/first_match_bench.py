#!/usr/bin/env python3
"""Same_color's first-mask labels for a batch, two routes on the same host inputs:
  (a) loop     one pipeline.label_points_first_match call per frame (set_camera, set_masks, a full run, clear_masks, the host pass):
               the only route before lpf_first_match; it takes at most 32 masks, so the rows with more have no baseline
  (b) batched  pipeline.first_match_frames: one lpf_first_match call per group of 256 masks for the whole batch
               (b_device: the same with the frames' masks already GPU tensors)
  (c) kernel   --kernel-only CASE: lpf_first_match alone on device-resident points, masks and outputs, for one
               `rocprofv3 --kernel-trace --stats` run of its own; --from-stats DIR turns that run into the kernels' us and the count
               kernel's GB/s on 16 B / point read plus the 4 B / point it writes (the mask reads are not counted)
Cases: golden20 (the 20 committed frames with their overlapping masks), full4x5 / full4x40 / full4x256 (the four full-size frames with
frame 100's five masks tiled out), synth8x2M (8 synthetic clouds of 2 M points, 5 masks; kernel route only).  The routes run in turn,
pass by pass, and agree on the first pass.  One JSON line per (case, route) with the library's build id, appended to --out.
  python tools/first_match_bench.py [--cases golden20,full4x5,full4x40,full4x256] [--passes 7] [--out profiles/first_match_bench.jsonl]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/first_match_bench.py --kernel-only CASE [--calls 10]
  python tools/first_match_bench.py --from-stats DIR --kernel-only CASE --points N"""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
FULL = ("frame_0000000100", "frame_0000001461_full", "frame_0000002098_full", "frame_0000002449_full")
CASES = ("golden20", "full4x5", "full4x40", "full4x256", "synth8x2M")
COUNT_BYTES = 16 + 4
HBM_PEAK = 8e12
DMAX = 30.0


class Cam:
    def __init__(self, calib):
        self.K, self.width, self.height = np.asarray(calib["K"], np.float64)[:3, :3], int(calib["width"]), int(calib["height"])


def frames_of(case, calib):
    """[(points, [M,H,W] uint8 masks)] of a case"""
    W = int(calib["width"])
    if case == "golden20":
        import first_match_ref as R
        idx = json.load(open(os.path.join(GOLDEN, "index.json")))["frames"]
        out = []
        for rec in idx:
            p, m = R.golden_frame_case(dict(np.load(os.path.join(GOLDEN, "frame_%010d.npz" % rec["frame"]))), calib)
            out.append((p, np.array(m, np.uint8).reshape(len(m), int(calib["height"]), W)))
        return out
    if case == "synth8x2M":
        from lidar_object_detection_amd import synthetic as S
        return [(sc["points"], np.ascontiguousarray(sc["masks"], dtype=np.uint8))
                for sc in (S.scene(2_000_000, n_masks=5, n_boxes=1, seed=40 + i) for i in range(8))]
    M = int(case.split("x")[1])
    five = np.unpackbits(np.load(os.path.join(GOLDEN, FULL[0] + ".npz"))["masks_rect5_packed"], axis=-1)[..., :W].astype(np.uint8)
    masks = np.stack([np.roll(five[i % 5], 8 * (i // 5), axis=1) for i in range(M)])
    return [(np.ascontiguousarray(np.load(os.path.join(GOLDEN, n + ".npz"))["points"], dtype=np.float32), masks) for n in FULL]


def spread(ts):
    return dict(ms_median=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3), passes=len(ts))


def end_to_end(case, calib, passes, warmup):
    import torch
    from lidar_object_detection_amd import pipeline
    cam, T = Cam(calib), np.asarray(calib["TrVeloToRect"])
    data = frames_of(case, calib)
    M = max(len(m) for _, m in data)
    cols = pipeline.default_colors(M)
    host = [pipeline.FrameInputs(i, p, m, colors=cols[:len(m)]) for i, (p, m) in enumerate(data)]
    dev = [pipeline.FrameInputs(i, p, torch.from_numpy(m).cuda(), colors=cols[:len(m)]) for i, (p, m) in enumerate(data)]
    ctx = pipeline.get_context(0)
    loop_ok = M <= pipeline.LPF_MAX_MASKS
    ta, tb, td = [], [], []
    for p in range(warmup + passes):
        want = None
        if loop_ok:
            t0 = time.perf_counter()
            want = [pipeline.label_points_first_match(f.points, T, cam, f.masks, f.colors, DMAX) for f in host]
            ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        got = pipeline.first_match_frames(host, T, cam, DMAX, ctx=ctx)
        tb.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        gdev = pipeline.first_match_frames(dev, T, cam, DMAX, ctx=ctx)
        td.append((time.perf_counter() - t0) * 1e3)
        if p == 0:                                           # the routes agree
            for f, g in enumerate(got):
                for k in ("car_idx", "car_mask", "background_idx", "colored_points", "colored_colors", "full_points"):
                    assert np.array_equal(g[k], gdev[f][k]), (f, k)
                    assert want is None or np.array_equal(g[k], want[f][k]), (f, k)
    base = dict(case=case, frames=len(data), masks_per_frame=M, points=int(sum(len(p) for p, _ in data)),
                car_points=int(sum(len(g["car_idx"]) for g in got)), background_points=int(sum(len(g["background_idx"]) for g in got)))
    rows = [dict(route="b_batched", total=spread(tb[warmup:]), **base), dict(route="b_batched_device_masks", total=spread(td[warmup:]), **base)]
    if loop_ok:
        rows.insert(0, dict(route="a_loop", total=spread(ta[warmup:]), **base))
        rows[1]["a_minus_b_pass_by_pass"] = spread([x - y for x, y in zip(ta[warmup:], tb[warmup:])])
    else:
        rows[0]["baseline"] = "none: label_points_first_match takes at most %d masks" % pipeline.LPF_MAX_MASKS
    return rows


def kernel_only(case, calib, calls):
    """lpf_first_match `calls` times on device-resident points, masks, colours and outputs (every output)"""
    import torch
    from lidar_object_detection_amd import pipeline
    cam = Cam(calib)
    data = frames_of(case, calib)
    ctx = pipeline.get_context(0)
    ctx.set_camera(np.asarray(calib["TrVeloToRect"]), cam.K, cam.width, cam.height, 0.0, DMAX)
    M = max(len(m) for _, m in data)
    batch = torch.zeros((len(data), M) + tuple(data[0][1].shape[1:]), dtype=torch.uint8, device="cuda")
    for i, (_, m) in enumerate(data):
        batch[i, :len(m)] = torch.from_numpy(m)
    colors = torch.rand((len(data), M, 3), dtype=torch.float64, device="cuda")
    staged = ctx.stage_points([p for p, _ in data])
    out = None
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls + 1):
        t0 = time.perf_counter()
        out = ctx.first_match(None, batch, colors, out=out and {k: v for k, v in out.items() if k != "frame_off"}, staged=staged)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(route="c_kernel_only", case=case, frames=len(data), masks_per_frame=M, points=int(staged[0][-1]), calls=calls,
                host_ms_per_call=spread(ts[1:]), car_points=int(out["n_car"].sum()), background_points=int(out["n_bg"].sum()))


def from_stats(dirs, case, points):
    w = csv.writer(sys.stdout)
    w.writerow(["case", "kernel", "calls", "avg_us", "min_us", "max_us", "points", "count_bytes_per_point", "GBps", "of_8TBps_peak"])
    for d in dirs:
        f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        for r in (csv.DictReader(open(f[-1])) if f else ()):
            if "lpf_fm_" not in r["Name"]:
                continue
            avg = float(r["AverageNs"]) / 1e3
            count = "lpf_fm_count" in r["Name"]
            bps = points * COUNT_BYTES / (avg * 1e-6) if count and points else 0.0
            w.writerow([case, r["Name"], r["Calls"], "%.2f" % avg, "%.2f" % (float(r["MinNs"]) / 1e3), "%.2f" % (float(r["MaxNs"]) / 1e3), points,
                        COUNT_BYTES if count else "", "%.1f" % (bps / 1e9) if count else "", "%.4f" % (bps / HBM_PEAK) if count else ""])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="golden20,full4x5,full4x40,full4x256")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-only", metavar="CASE", choices=CASES)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--from-stats", nargs="+", metavar="DIR")
    ap.add_argument("--points", type=int, default=0, help="--from-stats: points per call (the kernel-only line's points)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_match_bench.jsonl"))
    a = ap.parse_args()
    if a.from_stats:
        from_stats(a.from_stats, a.kernel_only or "synth8x2M", a.points)
        return
    from lidar_object_detection_amd import _build
    calib = dict(np.load(os.path.join(GOLDEN, "calib_cam0.npz")))
    lines = [kernel_only(a.kernel_only, calib, a.calls)] if a.kernel_only else [
        r for c in a.cases.split(",") for r in end_to_end(c, calib, a.passes, a.warmup)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in lines:
            r["source_id"] = _build.library_id(_build.LIB)
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
