"""One scan in two cameras with more than 32 masks: the multi-camera wide pass (lpf_run_cams_wide) against the route it replaces, on
the sample rig's cameras 0 and 1 (tests/golden: frame 100 and its camera-1 counterpart, the 5 detection masks tiled out to M).
Workloads: frame 100 and 20 copies of it as one batch, M = 40 / 64 / 128 per camera, and the mixed rig of 5 and 40 masks.

  default          wall time per call (median of --reps, the forms alternated in one process):
                     LpfContext.run_cams_wide vs two run_wide calls on two contexts (mixed: run_cams for the 5-mask camera + run_wide),
                     and the frame loop with the wide cameras in one run_cams_wide pass against run_frames_multicam (each camera
                     over 32 masks through run_frames on its own, the others in one run_cams pass)      -> profiles/multicam_wide_bench.jsonl
  --device-only    only the device forms, alternated, a marker kernel (torch's cos_) before each call, for rocprofv3:
                     rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python3 tools/multicam_wide_bench.py --device-only
                     rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <dir> -- python3 tools/multicam_wide_bench.py --device-only
  --from-trace F   kernel_trace.csv of the first run -> device time (sum of the lpf_* kernels) per call of each form, appended
  --from-pmc F     counter_collection.csv of the second (same --reps / --warmup) -> FETCH_SIZE of the projecting launches per workload

usage: python3 tools/multicam_wide_bench.py [--reps 20] [--warmup 3] [--device-only | --from-trace F | --from-pmc F]"""
import argparse
import collections
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cam1_fixtures import load_calib1, load_cam1_golden                 # noqa: E402
from conftest import load_calib, load_golden, unpack_masks             # noqa: E402
from lidar_object_detection_amd import kitti360, pipeline               # noqa: E402

OUT = os.path.join(ROOT, "profiles", "multicam_wide_bench.jsonl")
FRAMES = (("frame100", 1), ("20frames", 20))
MASKS = ((40, 40), (64, 64), (128, 128), (5, 40))
WORKLOADS = [(name, F, ms) for name, F in FRAMES for ms in MASKS]
FLAGS = dict(want_uv=False, want_valid_uv=True)                         # what run_frames_multicam asks for


def _rig():
    c0, c1 = load_calib(), load_calib1()
    g0, g1 = load_golden(100), load_cam1_golden(100)
    cams = []
    for cal, g, rr in ((c0, g0, "R_rect"), (c1, g1, "R_rect_01")):
        cam = kitti360.CameraPerspective.from_arrays(cal["K"], cal[rr], int(cal["width"]), int(cal["height"]))
        cams.append(dict(T=np.asarray(cal["TrVeloToRect"]), cam=cam, base=unpack_masks(g, "rect5", cam.height, cam.width).astype(np.uint8),
                         corners=g["corners_velo"]))
    return g0["points"], cams


def _tiled(base, M):
    """M masks out of the camera's 5: copies shifted sideways (the tiling of test_wide_golden_frame_100)"""
    W = base.shape[2]
    return np.stack([np.roll(base[i % len(base)], shift=(7 * (i // len(base))) % W, axis=1) for i in range(M)])


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


def _device_forms(torch, pts, cams, F, ms):
    """{form: callable} over the same inputs in HBM: the wide pass, today's route and (mixed rig) the split route"""
    from lidar_object_detection_amd._native import LpfContext
    dev = torch.device("cuda", 0)
    pts_d = torch.from_numpy(np.ascontiguousarray(np.concatenate([pts] * F))).to(dev)
    n = len(pts)
    frames = [pts_d] if F == 1 else [pts_d[i * n:(i + 1) * n] for i in range(F)]
    masks = [torch.from_numpy(np.ascontiguousarray(np.stack([_tiled(c["base"], M)] * F))).to(dev) for c, M in zip(cams, ms)]
    boxes = [[c["corners"]] * F for c in cams]
    specs = [dict(T_velo_to_rect=c["T"], K=c["cam"].K, width=c["cam"].width, height=c["cam"].height, masks=m, boxes=b)
             for c, m, b in zip(cams, masks, boxes)]
    cx = LpfContext(0)
    singles = [LpfContext(0) for _ in cams]
    for s, c in zip(singles, cams):
        s.set_camera(c["T"], c["cam"].K, c["cam"].width, c["cam"].height, 0.0, 50.0)

    # an instance-list capacity that fits every camera's lists: each call of every form is one native pass (with the default, the
    # 128-mask lists overflow and every form runs twice)
    first = cx.run_cams_wide(frames, specs, **FLAGS)
    cap = max(sum(len(l) for l in r["inst_lists"]) for rc in first for r in rc) + 1
    flags = dict(FLAGS, inst_cap=cap)

    def one_pass():
        return cx.run_cams_wide(frames, specs, **flags)

    def today():                                       # before lpf_run_cams_wide: a narrow camera in run_cams, each wide one in run_wide
        out = []
        for k, (s, m, b, M) in enumerate(zip(singles, masks, boxes, ms)):
            if M <= 32:
                out.append(cx.run_cams(frames, [specs[k]], want_label=False, pinned=True, **flags)[0])
            else:
                s.set_boxes(b)
                out.append(s.run_wide(frames, m, **flags))
        return out

    def split():                                       # the narrow camera in run_cams, the wide ones in one run_cams_wide pass
        narrow = [k for k, M in enumerate(ms) if M <= 32]
        wide = [k for k, M in enumerate(ms) if M > 32]
        out = {}
        out.update(zip(narrow, cx.run_cams(frames, [specs[k] for k in narrow], want_label=False, pinned=True, **flags)))
        out.update(zip(wide, cx.run_cams_wide(frames, [specs[k] for k in wide], **flags)))
        return [out[k] for k in range(len(ms))]

    forms = dict(pass_=one_pass, today=today)
    if min(ms) <= 32:
        forms["split"] = split
    ref = one_pass()
    for name, f in forms.items():                      # every form computes the same
        got = f()
        for k in range(len(cams)):
            for x, y in zip(got[k], ref[k]):
                assert np.array_equal(x["valid_idx"], y["valid_idx"]) and np.array_equal(x["count_mb"], y["count_mb"]), name
                assert all(np.array_equal(p, q) for p, q in zip(x["inst_lists"], y["inst_lists"])), name
    return forms


def _wide_route(per_cam, rig, ctx):
    """The frame loop as it would be with the wide pass: the cameras of more than 32 masks (up to 256) in ONE run_cams_wide pass,
    the others through run_frames_multicam (one run_cams pass) -- what run_frames_multicam does not do"""
    out, wide = {}, []
    for k, (T, cam) in enumerate(rig):
        if max(len(f.masks) for f in per_cam[k]) <= 32:
            continue
        ctx.set_camera(T, cam.K, cam.width, cam.height, 0.0, 50.0)
        stacks, er, v3 = pipeline._frame_mask_stacks(per_cam[k], cam, ctx, 0, False)
        counts = [s_.shape[0] for s_ in stacks]
        corners, pos = zip(*(pipeline._corners_velo(f.bboxes_3d) for f in per_cam[k]))
        wide.append((k, counts, pos, dict(T_velo_to_rect=T, K=cam.K, width=cam.width, height=cam.height, depth_max=50.0,
                                          masks=pipeline._mask_batch(stacks, max(counts), cam.height, cam.width, ctx), erode_iters=er,
                                          binarize="v3" if v3 else "astype", boxes=list(corners))))
    if wide:
        res = ctx.run_cams_wide([f.points for f in per_cam[wide[0][0]]], [w[3] for w in wide], want_uv=False, want_label=False,
                                want_valid_uv=True, pinned=True)
        for (k, counts, pos, _), rc in zip(wide, res):
            out[k] = [pipeline._frame_result(f, r, m, p, 10, True) for f, r, m, p in zip(per_cam[k], rc, counts, pos)]
    narrow = [k for k in range(len(per_cam)) if k not in out]
    if narrow:
        out.update(zip(narrow, pipeline.run_frames_multicam([per_cam[k] for k in narrow], [rig[k] for k in narrow], ctx=ctx)))
    return [out[k] for k in range(len(per_cam))]


def wall(reps, warmup):
    import torch
    pts, cams = _rig()
    lines = []
    for name, F, ms in WORKLOADS:
        forms = _device_forms(torch, pts, cams, F, ms)
        t = _median_ms(forms, reps, warmup)
        lines.append(dict(what="run_cams_wide (2 cameras) vs today's route (two run_wide; mixed: run_cams + run_wide), inputs in HBM",
                          workload=name, frames=F, masks=list(ms), points_per_frame=len(pts), ms=t,
                          speedup_vs_today=t["today"] / t["pass_"]))
        per_cam = [[pipeline.FrameInputs(100, pts, _tiled(c["base"], M), [{"corners_velo": x.tolist()} for x in c["corners"]],
                                         pipeline.default_colors(M)) for _ in range(F)] for c, M in zip(cams, ms)]
        rig = [(c["T"], c["cam"]) for c in cams]
        ctx = pipeline.get_context(0)

        fns = {"wide_pass": lambda: _wide_route(per_cam, rig, ctx), "run_frames_multicam": lambda: pipeline.run_frames_multicam(per_cam, rig, ctx=ctx)}
        t = _median_ms(fns, reps, warmup)
        lines.append(dict(what="the frame loop with a run_cams_wide pass vs run_frames_multicam (wide cameras through run_frames; host points, same context)",
                          workload=name, frames=F, masks=list(ms), ms_per_frame={k: v / F for k, v in t.items()},
                          speedup=t["run_frames_multicam"] / t["wide_pass"]))
    return lines


def device_only(reps, warmup):
    import torch
    pts, cams = _rig()
    mark = torch.zeros(1, device=torch.device("cuda", 0))
    for name, F, ms in WORKLOADS:
        mark.cos_()                                    # (the set-up's calls: a segment of their own, left out)
        forms = _device_forms(torch, pts, cams, F, ms)
        for _ in range(warmup + reps):                 # alternated; a marker kernel before each call (--from-trace segments on it)
            for f in forms.values():
                mark.cos_()
                f()
    torch.cuda.synchronize()
    print("device-only done")


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def _col(r, *names):
    for n in names:
        if n in r:
            return r[n]
    raise KeyError(names)


def _short(name):
    return name.split("(")[0].split("<")[0].replace("void ", "")


def _segments(rows, reps, warmup, keep):
    """Rows of a rocprofv3 CSV in start order, cut at the marker kernels -> {(workload, form): [per call: [row, ...]]} of the rows
    keep(row) accepts (warm-up calls and each workload's set-up segment left out)"""
    rows = sorted(rows, key=lambda r: int(_col(r, "Start_Timestamp")))
    segs, cur = [], None
    for r in rows:
        name = _col(r, "Kernel_Name")
        if "cos_kernel" in name:                       # (the marker: torch's cos, which nothing else here launches)
            if cur is not None:
                segs.append(cur)
            cur = []
        elif cur is not None and keep(r):
            cur.append(r)
    if cur is not None:
        segs.append(cur)
    out, i = {}, 0
    for name, F, ms in WORKLOADS:
        forms = ["pass_", "today", "split"][:3 if min(ms) <= 32 else 2]
        i += 1                                         # the set-up segment
        block = segs[i:i + len(forms) * (warmup + reps)]
        i += len(forms) * (warmup + reps)
        for j, form in enumerate(forms):
            out[(name, F, tuple(ms), form)] = block[j::len(forms)][warmup:]
    return out


def from_trace(path, reps, warmup):
    """Device time per call of each form: the sum of its lpf_* kernels (memsets and copies left out)."""
    seg = _segments(_rows(path), reps, warmup, lambda r: _col(r, "Kernel_Name").startswith(("lpf_", "void lpf_")))
    lines = []
    for name, F, ms in WORKLOADS:
        d = {}
        for (w, f, m, form), calls in seg.items():
            if (w, f, m) != (name, F, tuple(ms)):
                continue
            dur = [[(_short(_col(r, "Kernel_Name")), (int(_col(r, "End_Timestamp")) - int(_col(r, "Start_Timestamp"))) / 1e3) for r in c]
                   for c in calls]
            us = collections.defaultdict(list)
            for c in dur:
                tot = collections.defaultdict(float)
                for n, t in c:
                    tot[n] += t
                for n, t in tot.items():
                    us[n].append(t)
            d[form] = dict(us_kernel_sum=float(np.median([sum(t for _, t in c) for c in dur])), launches=len(dur[0]),
                           by_kernel=dict(collections.Counter(n for n, _ in dur[0])),
                           us_by_kernel={n: round(float(np.median(v)), 2) for n, v in us.items()})
        lines.append(dict(what="device time per call (rocprofv3, sum of the lpf_* kernels, forms alternated in one process, inst_cap that fits)",
                          workload=name, frames=F, masks=list(ms), samples=reps, forms=d,
                          kernel_sum_ratio_today_over_pass=d["today"]["us_kernel_sum"] / d["pass_"]["us_kernel_sum"]))
    return lines


def from_pmc(path, reps, warmup):
    """FETCH_SIZE per workload: the pass's projecting launch against each projecting launch of today's route (one per camera)."""
    proj = ("lpf_cams_wide_project", "lpf_wide_project", "lpf_cams_stream")
    seg = _segments(_rows(path), reps, warmup, lambda r: _col(r, "Counter_Name") == "FETCH_SIZE" and _short(_col(r, "Kernel_Name")) in proj)
    lines = []
    for name, F, ms in WORKLOADS:
        d = {}
        for form in ("pass_", "today"):
            kb = collections.defaultdict(list)
            for c in seg[(name, F, tuple(ms), form)]:
                for r in c:
                    kb[_short(_col(r, "Kernel_Name"))].append(float(_col(r, "Counter_Value")))
            d[form] = {k: dict(fetch_kb=float(np.median(v)), launches_per_call=len(v) // max(1, len(seg[(name, F, tuple(ms), form)])))
                       for k, v in kb.items()}
        n = 109355 * F
        lines.append(dict(what="FETCH_SIZE (KB) of the projecting launches per call, median over calls (16 B of points per point)", workload=name,
                          frames=F, masks=list(ms), points=n, points_kb=16 * n / 1024, forms=d))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--from-trace")
    ap.add_argument("--from-pmc")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.device_only:
        return device_only(a.reps, a.warmup)
    lines = (from_trace(a.from_trace, a.reps, a.warmup) if a.from_trace else from_pmc(a.from_pmc, a.reps, a.warmup) if a.from_pmc
             else wall(a.reps, a.warmup))
    with open(a.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
