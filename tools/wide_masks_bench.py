"""Frames with more than 32 detections: the native wide pass (lpf_run_wide through pipeline.run_frames) against the per-group
passes of pipeline._run_frames_in_mask_groups (one narrow run per 32 masks), on sample frame 100's scan with its 5 detection masks
tiled (shifted copies) out to M masks.  Prints one JSON line per M: wall time per call (median of --reps) of each path, and of the
bare LpfContext.run_wide call.  Device time: run this under rocprofv3 --kernel-trace --stats (tools/wide_masks_bench.py --reps 20).

usage: python3 tools/wide_masks_bench.py [--masks 40,64,128,256] [--reps 30] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import load_calib, load_golden, unpack_masks            # noqa: E402
from lidar_object_detection_amd import kitti360, pipeline            # noqa: E402


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", default="40,64,128,256")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    calib = load_calib()
    cam = kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))
    g = load_golden(100)
    base = unpack_masks(g, "rect5", cam.height, cam.width).astype(np.uint8)
    boxes = [{"corners_velo": c.tolist()} for c in g["corners_velo"]]
    ctx = pipeline.get_context(0)
    for M in [int(x) for x in a.masks.split(",")]:
        mk = np.stack([np.roll(base[i % len(base)], 7 * (i // len(base)), axis=1) for i in range(M)])
        fi = [pipeline.FrameInputs(100, g["points"], mk, boxes)]
        wide = lambda: pipeline.run_frames(fi, calib["TrVeloToRect"], cam, 50.0, 10, True)     # noqa: E731
        def grouped():                        # what run_frames did for M > 32 before the wide pass: the mask stack, then a run per 32 masks
            stacks = [pipeline._mask_stack(mk, cam, resize_ctx=ctx)[0]]
            return pipeline._run_frames_in_mask_groups(fi, stacks, calib["TrVeloToRect"], cam, 50.0, 10, True, 0, False, 0, ctx)
        t_wide = _median_ms(wide, a.reps, a.warmup)
        t_grp = _median_ms(grouped, a.reps, a.warmup)
        c = pipeline.get_context(0)
        t_call = _median_ms(lambda: c.run_wide([g["points"]], mk, want_uv=False, want_valid_uv=True), a.reps, a.warmup)
        print(json.dumps(dict(M=M, points=int(len(g["points"])), boxes=len(boxes), run_frames_wide_ms=round(t_wide, 3),
                              mask_groups_ms=round(t_grp, 3), run_wide_call_ms=round(t_call, 3), speedup=round(t_grp / t_wide, 2))),
              flush=True)


if __name__ == "__main__":
    main()
