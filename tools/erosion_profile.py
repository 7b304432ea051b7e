#!/usr/bin/env python3
"""Kernel times of the mask pack and erosion at one erosion element size (lpf_set_erosion_element), for DESIGN section 20.

  rocprofv3 --kernel-trace --stats -f csv -d OUT -o k<K>_<CASE> -- python tools/erosion_profile.py run K CASE
      set_masks + run_batch, 60 times, with the K x K element.  CASE: A = 8 masks at 1408 x 376, F = 1, 1 iteration (bench.py's
      configs[4] mask shape); B1 / B2 = a batch of F = 20 frames of M = 5 masks, 1 / 2 iterations.  One profiler run per (K, CASE):
      the kernels of the shapes share their names.
  python tools/erosion_profile.py summary OUT [CSV]
      the pack / erosion rows of OUT's k*_kernel_stats.csv files as one table (and as CSV: profiles/erosion_element_kernel_stats.csv)."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"A": "8 masks 1408x376 F=1 1 iteration", "B1": "F=20 M=5 1 iteration", "B2": "F=20 M=5 2 iterations"}


def run(k, case):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from lidar_object_detection_amd import synthetic as S
    from lidar_object_detection_amd._native import LpfContext
    F, M, iters, n = {"A": (1, 8, 1, 1_000_000), "B1": (20, 5, 1, 120_000), "B2": (20, 5, 2, 120_000)}[case]
    calib = dict(np.load(os.path.join(ROOT, "tests", "golden", "calib_cam0.npz")))
    _, T, K, W, H = S.default_calibration(calib)
    scs = [S.scene(n, M, 8, seed=10 + f, calib=calib) for f in range(min(F, 4))]
    masks = torch.from_numpy(np.stack([scs[f % len(scs)]["masks"] for f in range(F)])).cuda()
    pts = [torch.from_numpy(scs[f % len(scs)]["points"]).cuda() for f in range(F)]
    torch.cuda.synchronize()
    with LpfContext(0) as c:
        c.set_camera(T, K, W, H, 0.0, 50.0)
        c.set_erosion_element(k)
        c.set_boxes([scs[f % len(scs)]["corners_velo"] for f in range(F)], oriented=True)
        for _ in range(60):
            c.set_masks(masks, erode_iters=iters)
            r = c.run_batch(pts, want_uv=False, want_label=False, want_valid_uv=True)
        c.sync()
    print("k=%d case=%s F=%d M=%d iters=%d labelled=%d" % (k, case, F, M, iters, sum(x["n_labelled"] for x in r)), flush=True)


def summary(out, csv_path=None):
    rows = []
    for path in sorted(glob.glob(os.path.join(out, "**", "*_kernel_stats.csv"), recursive=True)):
        m = re.search(r"k(\d+)_(A|B1|B2)_kernel_stats", os.path.basename(path))
        if not m:
            continue
        k, case = int(m.group(1)), m.group(2)
        with open(path) as f:
            for r in csv.DictReader(f):
                if re.search(r"lpf_(pack|erode|wide_pack)", r["Name"]):
                    rows.append((case, k, r["Name"], int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))
    rows.sort(key=lambda t: (t[0], t[1], t[2]))
    table = [[CASES[case], k, name, calls, "%.2f" % avg, "%.2f" % mn, "%.2f" % mx] for case, k, name, calls, avg, mn, mx in rows]
    for t in table:
        print("%-34s k=%2d %-90s calls %4d avg %8s us  min %8s  max %8s" % (t[0], t[1], t[2][:90], t[3], t[4], t[5], t[6]))
    if csv_path:
        with open(csv_path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["case", "ksize", "kernel", "calls", "avg_us", "min_us", "max_us"])
            w.writerows(table)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "summary":
        summary(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        raise SystemExit(__doc__)
