"""One scan in two cameras: the multi-camera pass (lpf_run_cams) against the two single-camera runs it replaces, on the sample rig's
cameras 0 and 1 with their 5 detection masks each (tests/golden: frame 100 and its camera-1 counterpart).  Two workloads: frame 100,
and 20 copies of it as one batch (bench.py's configs[3] shape).

  default          wall time per call (median of --reps, the two forms alternated): LpfContext.run_cams vs run_batch on two contexts
                   (one per camera), run_frames_multicam vs two run_frames, process_frames_multicam vs two process_frames (per
                   frame, over a dataset tree of 20 frames rebuilt from the fixtures) -> profiles/multicam_bench.jsonl
  --device-only    only the pass / two-run alternation, for rocprofv3 (nothing else on the GPU in between):
                     rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/multicam_bench.py --device-only
                     rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- python3 tools/multicam_bench.py --device-only
  --from-trace F   kernel_trace.csv of the first run -> device time per pass / per two runs (sums of kernel durations) and launches
                   per pass, appended to profiles/multicam_bench.jsonl
  --from-pmc F     counter_collection.csv of the second -> FETCH_SIZE of the streaming launches, appended likewise

usage: python3 tools/multicam_bench.py [--reps 30] [--warmup 3] [--device-only | --from-trace F | --from-pmc F]"""
import argparse
import collections
import contextlib
import csv
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cam1_fixtures import load_calib1, load_cam1_golden                 # noqa: E402
from conftest import load_calib, load_golden, unpack_masks             # noqa: E402
from lidar_object_detection_amd import kitti360, pipeline               # noqa: E402

OUT = os.path.join(ROOT, "profiles", "multicam_bench.jsonl")
WORKLOADS = (("frame100", 1), ("20frames", 20))
FLAGS = dict(want_uv=False, want_label=False, want_valid_uv=True, pinned=True)      # what run_frames asks for


def _rig():
    c0, c1 = load_calib(), load_calib1()
    g0, g1 = load_golden(100), load_cam1_golden(100)
    cams = []
    for cal, g, rr in ((c0, g0, "R_rect"), (c1, g1, "R_rect_01")):
        cam = kitti360.CameraPerspective.from_arrays(cal["K"], cal[rr], int(cal["width"]), int(cal["height"]))
        cams.append(dict(T=np.asarray(cal["TrVeloToRect"]), cam=cam, masks=unpack_masks(g, "rect5", cam.height, cam.width).astype(np.uint8),
                         corners=g["corners_velo"], g=g))
    return g0["points"], cams


def _median_ms(fns, reps, warmup):
    """fns: {name: callable}, run alternately; median wall ms of each"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    t = collections.defaultdict(list)
    for _ in range(reps):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    return {k: 1e3 * float(np.median(v)) for k, v in t.items()}


def _device_forms(torch, pts, cams, F):
    """(pass, two runs): the same inputs, in HBM, for both forms"""
    from lidar_object_detection_amd._native import LpfContext
    dev = torch.device("cuda", 0)
    pts_d = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts] * F))).to(dev)
    n = len(pts)
    frames = [pts_d] if F == 1 else [pts_d[i * n:(i + 1) * n] for i in range(F)]
    masks = [torch.from_numpy(np.ascontiguousarray(np.stack([c["masks"]] * F))).to(dev) for c in cams]
    boxes = [[c["corners"]] * F for c in cams]
    cx = LpfContext(0)
    singles = [LpfContext(0) for _ in cams]
    for s, c in zip(singles, cams):
        s.set_camera(c["T"], c["cam"].K, c["cam"].width, c["cam"].height, 0.0, 50.0)
    specs = [dict(T_velo_to_rect=c["T"], K=c["cam"].K, width=c["cam"].width, height=c["cam"].height, masks=m, boxes=b)
             for c, m, b in zip(cams, masks, boxes)]

    def one_pass():
        return cx.run_cams(frames, specs, **FLAGS)

    def two_runs():
        out = []
        for s, m, b in zip(singles, masks, boxes):
            s.set_masks(m, lend=True)
            s.set_boxes(b)
            out.append(s.run_batch(frames, **FLAGS))
        return out

    a, b = one_pass(), two_runs()
    for k in range(len(cams)):
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(x["valid_idx"], y["valid_idx"]) and np.array_equal(x["count_mb"], y["count_mb"])
            assert all(np.array_equal(p, q) for p, q in zip(x["inst_lists"], y["inst_lists"]))
    return one_pass, two_runs


def _tree(root, pts, cams, nframes):
    seq = "2013_05_28_drive_0000_sync"
    g = cams[0]["g"]
    (root / "data_3d_raw" / seq / "velodyne_points" / "data").mkdir(parents=True)
    (root / "bboxes_3D_cam0").mkdir()
    raw = json.dumps([{"index": int(i), "corners_cam0": c.tolist()} for i, c in zip(g["box_index_raw"], g["corners_cam0_raw"])])
    for c in range(len(cams)):
        (root / "data_2d_raw" / seq / ("image_%02d" % c) / "data_rect").mkdir(parents=True)
    for f in range(nframes):
        pts.tofile(str(root / "data_3d_raw" / seq / "velodyne_points" / "data" / ("%010d.bin" % f)))
        (root / "bboxes_3D_cam0" / ("BBoxes_%d.json" % f)).write_text(raw)
        for c in range(len(cams)):
            (root / "data_2d_raw" / seq / ("image_%02d" % c) / "data_rect" / ("%010d.png" % f)).write_bytes(b"")
    return seq


def wall(reps, warmup):
    import pathlib
    import torch
    pts, cams = _rig()
    lines = []
    for name, F in WORKLOADS:
        one_pass, two_runs = _device_forms(torch, pts, cams, F)
        t = _median_ms({"pass": one_pass, "two_runs": two_runs}, reps, warmup)
        lines.append(dict(what="LpfContext.run_cams (2 cameras) vs run_batch on two contexts, inputs in HBM", workload=name, frames=F,
                          points_per_frame=len(pts), masks_per_camera=5, ms_pass=t["pass"], ms_two_runs=t["two_runs"],
                          speedup=t["two_runs"] / t["pass"]))
        per_cam = [[pipeline.FrameInputs(100, pts, c["masks"], [{"corners_velo": x.tolist()} for x in c["corners"]],
                                         pipeline.default_colors(5)) for _ in range(F)] for c in cams]
        rig = [(c["T"], c["cam"]) for c in cams]
        ctx = pipeline.get_context(0)
        t = _median_ms({"multicam": lambda: pipeline.run_frames_multicam(per_cam, rig, ctx=ctx),
                        "two_calls": lambda: [pipeline.run_frames(per_cam[k], *rig[k], ctx=ctx) for k in range(len(rig))]}, reps, warmup)
        lines.append(dict(what="run_frames_multicam vs two run_frames (host points, same context)", workload=name, frames=F,
                          ms_per_frame_multicam=t["multicam"] / F, ms_per_frame_two_calls=t["two_calls"] / F,
                          speedup=t["two_calls"] / t["multicam"]))
    nframes = 20
    with tempfile.TemporaryDirectory() as tmp:
        root = pathlib.Path(tmp) / "KITTI360_sample"
        seq = _tree(root, pts, cams, nframes)
        velo = kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=str(root))
        calib = {0: load_calib(), 1: load_calib1()}
        orig = pipeline.sequence_setup
        pipeline.sequence_setup = lambda path, s=0, c=0: (seq, cams[c]["cam"], calib[c]["TrVeloToCam"], cams[c]["T"], velo)
        seg = lambda p: (None, cams[int(os.path.basename(os.path.dirname(os.path.dirname(p)))[-2:])]["masks"],      # noqa: E731
                         pipeline.default_colors(5), np.zeros((5, 4), np.float32), np.ones(5))
        k = [0]

        def csvs():
            k[0] += 1
            return {c: os.path.join(tmp, "r%d" % k[0], "cam%d.csv" % c) for c in (0, 1)}

        def multi():
            with contextlib.redirect_stdout(io.StringIO()):
                pipeline.process_frames_multicam(0, (0, 1), segmenter=seg, image_loader=lambda p: p, kitti360_path=str(root),
                                                 master_csv_paths=csvs(), timestamp="T")

        def two():
            paths = csvs()
            with contextlib.redirect_stdout(io.StringIO()):
                for c in (0, 1):
                    pipeline.process_frames(0, c, segmenter=seg, image_loader=lambda p: p, kitti360_path=str(root),
                                            master_csv_path=paths[c], timestamp="T")
        try:
            t = _median_ms({"multicam": multi, "two_calls": two}, max(3, reps // 6), 1)
        finally:
            pipeline.sequence_setup = orig
        lines.append(dict(what="process_frames_multicam vs two process_frames (files -> CSVs, read-ahead reader)", workload="20 files of frame 100",
                          frames=nframes, ms_per_frame_multicam=t["multicam"] / nframes, ms_per_frame_two_calls=t["two_calls"] / nframes,
                          speedup=t["two_calls"] / t["multicam"]))
    return lines


def device_only(reps, warmup):
    import torch
    pts, cams = _rig()
    for name, F in WORKLOADS:
        one_pass, two_runs = _device_forms(torch, pts, cams, F)
        for _ in range(warmup + reps):                   # strictly alternated: pass, two runs, pass, ... (--from-trace relies on it)
            one_pass()
            two_runs()
    print("device-only done")


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def _col(r, *names):
    for n in names:
        if n in r:
            return r[n]
    raise KeyError(names)


def from_trace(path, reps, warmup):
    """Segments the kernels in start order: a pass ends with lpf_cams_finalize, two runs with their second lpf_finalize."""
    rows = sorted(_rows(path), key=lambda r: int(_col(r, "Start_Timestamp", "start")))
    segs, cur, fin = [], [], 0
    for r in rows:
        name = _col(r, "Kernel_Name", "kernel_name")
        if not name.startswith(("lpf_", "void lpf_")) or "lpf_results_to_host" in name:
            continue                                        # (result delivery into page-locked host memory: the same in both forms)
        cur.append((name, int(_col(r, "Start_Timestamp")), int(_col(r, "End_Timestamp"))))
        if "lpf_cams_finalize" in name:
            segs.append(("pass", cur)); cur = []
        elif "lpf_finalize" in name:
            fin += 1
            if fin == 2:
                segs.append(("two_runs", cur)); cur, fin = [], 0
    lines = []
    per = 2 * (warmup + reps) + 2                           # (+ the check of _device_forms: one pass, two runs)
    for w, (name, F) in enumerate(WORKLOADS):
        part = segs[w * per:(w + 1) * per][2 + 2 * warmup:]
        d = {}
        for kind in ("pass", "two_runs"):
            ks = [s for k, s in part if k == kind]
            sums = [sum(e - b for _, b, e in s) / 1e3 for s in ks]
            spans = [(max(e for _, _, e in s) - min(b for _, b, _ in s)) / 1e3 for s in ks]
            names = collections.Counter(n.split("(")[0].split("<")[0].replace("void ", "") for n, _, _ in ks[0])
            us = collections.defaultdict(list)
            for s in ks:
                tot = collections.defaultdict(float)
                for n, b, e in s:
                    tot[n.split("(")[0].split("<")[0].replace("void ", "")] += (e - b) / 1e3
                for n, v in tot.items():
                    us[n].append(v)
            d[kind] = dict(us_kernel_sum=float(np.median(sums)), us_span=float(np.median(spans)), launches=len(ks[0]), by_kernel=dict(names),
                           us_by_kernel={n: float(np.median(v)) for n, v in us.items()})
        lines.append(dict(what="device time per pass vs two single-camera runs (rocprofv3 kernel sums, alternated in one process)",
                          workload=name, frames=F, samples=len(part) // 2, pass_=d["pass"], two_runs=d["two_runs"],
                          kernel_sum_ratio=d["two_runs"]["us_kernel_sum"] / d["pass"]["us_kernel_sum"]))
    return lines


def from_pmc(path):
    rows = _rows(path)
    acc = collections.defaultdict(list)
    for r in rows:
        name = _col(r, "Kernel_Name")
        if _col(r, "Counter_Name") != "FETCH_SIZE" or not ("lpf_cams_stream" in name or "lpf_step_t" in name or "lpf_k1_project_t" in name):
            continue
        acc[(name.split("(")[0].replace("void ", ""), int(_col(r, "Grid_Size")))].append(float(_col(r, "Counter_Value")))
    return [dict(what="FETCH_SIZE (KB) per streaming launch, median over dispatches", kernel=k, grid_size=g, fetch_kb=float(np.median(v)),
                 dispatches=len(v)) for (k, g), v in sorted(acc.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--from-trace")
    ap.add_argument("--from-pmc")
    a = ap.parse_args()
    if a.device_only:
        return device_only(a.reps, a.warmup)
    if a.from_trace or a.from_pmc:
        lines = from_trace(a.from_trace, a.reps, a.warmup) if a.from_trace else from_pmc(a.from_pmc)
        mode = "a"
    else:
        lines = wall(a.reps, a.warmup)
        mode = "w"
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, mode) as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
