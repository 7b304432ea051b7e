#!/usr/bin/env python3
"""Generate tests/golden/depth_overlays_golden.json and tests/golden/jet_lut_u8.npy from the REFERENCE's own statements.

Runs only where the reference checkout of make_golden.py (make_golden.REF) exists.  Nothing from the reference is copied: its lines
are sliced out of seg_with_pointcloud.py at generation time (make_golden.run_ref) and executed on this script's variables.

For each of the 23 golden frames (the 20 sample frames, and frames 1461, 2098 and 2449 at full size) and each mask set (rect5, edge):
  * the projection :132-139 and the per-car depth maps :154-170 (depth < 30), the script's literal loop;
    frame 100's rect5 maps are checked against the reference lists committed by make_golden.py (depthmap_*_rect5);
  * the overlay statements :173-180, once per car, with the real plt.get_cmap('jet') and a cv2 stub whose
    cvtColor(x, COLOR_RGB2BGR) is x[..., ::-1], on a seeded segmented image per frame (tests/overlay_ref.seg_image).
Written per car: the overlay's SHA-256, np.max(depthMap) as a float hex string, the skipped flag and the pixel count; plus the seeds,
the matplotlib version and the 256 x 3 uint8 table (cm._lut[:256, :3] * 255).astype(np.uint8).

Usage: python tests/golden/make_golden_overlays.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import matplotlib  # noqa: E402
matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

import make_golden  # noqa: E402
import overlay_ref as R  # noqa: E402
from conftest import load_calib  # noqa: E402
from lidar_object_detection_amd import kitti360  # noqa: E402

SCRIPT = "seg_with_pointcloud.py"


def _cv2_stub():
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2BGR = 4

    def cvtColor(x, code):
        assert code == cv2.COLOR_RGB2BGR and x.dtype == np.uint8 and x.shape[-1] == 3
        return x[..., ::-1]

    cv2.cvtColor = cvtColor
    return cv2


def main():
    camera = kitti360.CameraPerspective(make_golden.DATA, make_golden.SEQ, 0)
    cal = load_calib()
    T = np.asarray(cal["TrVeloToRect"], np.float64)
    H, W = int(camera.height), int(camera.width)
    assert (H, W) == (int(cal["height"]), int(cal["width"]))
    cm = plt.get_cmap("jet")
    cm(0.5)                                                     # (builds _lut)
    lut = (cm._lut[:256, :3] * 255).astype(np.uint8)
    np.save(os.path.join(HERE, "jet_lut_u8.npy"), lut)
    cv2 = _cv2_stub()

    inputs = R.golden_inputs(H, W)
    frames = []
    for key, d in inputs.items():
        rec = dict(key=key, frame=d["frame"], full=d["full"], seg_seed=R.SEG_SEED + d["frame"] + (R.FULL_SEED_OFFSET if d["full"] else 0))
        ns = {"np": np, "points": d["pts"].copy(), "TrVeloToRect": T, "camera": camera}
        make_golden.run_ref(SCRIPT, 132, 139, ns, "points[:, 3] = 1")
        for kind in ("rect5", "edge"):
            masks = d[kind].astype(np.float32)
            ns.update(masks=masks)
            make_golden.run_ref(SCRIPT, 154, 170, ns, "valid = np.logical_and.reduce((")
            maps = ns["per_car_depth_maps"]
            if kind == "rect5" and key == "100":                # the reference lists committed by make_golden.py
                g = np.load(os.path.join(HERE, "frame_0000000100.npz"))
                idx, val, off = g["depthmap_idx_rect5"], g["depthmap_val_rect5"], g["depthmap_off_rect5"]
                for m, (_, dm) in enumerate(maps):
                    p = np.flatnonzero(dm)
                    assert np.array_equal(p, idx[off[m]:off[m + 1]]) and np.array_equal(dm.ravel()[p], val[off[m]:off[m + 1]])
            cars = []
            for car_id, depthMap in maps:
                ons = {"np": np, "cv2": cv2, "cm": cm, "masking_image": d["seg"], "per_car_depth_maps": [(car_id, depthMap)],
                       "image_withseg": None}
                make_golden.run_ref(SCRIPT, 173, 180, ons, "for car_id, depthMap in per_car_depth_maps:")
                img = ons["image_withseg"]
                p = np.flatnonzero(depthMap)
                mine, mx = R.overlay(d["seg"], p, depthMap.ravel()[p], lut)
                assert mx == float(np.max(depthMap))
                if img is not None:
                    assert np.array_equal(img, mine), (key, kind, car_id)
                cars.append(dict(car_id=int(car_id), skipped=img is None, n_pixels=int(len(p)), max_hex=float(np.max(depthMap)).hex(),
                                 sha256=None if img is None else R.sha(img)))
            rec[kind] = cars
        frames.append(rec)
        print("%-10s rect5 %d cars (%d skipped), edge %d cars (%d skipped)" % (
            key, len(rec["rect5"]), sum(c["skipped"] for c in rec["rect5"]), len(rec["edge"]), sum(c["skipped"] for c in rec["edge"])))
    out = dict(script=SCRIPT + ":132-180", matplotlib=matplotlib.__version__, seg_seed=R.SEG_SEED, full_seed_offset=R.FULL_SEED_OFFSET,
               depth_max=R.DMAX, H=H, W=W, frames=frames)
    with open(os.path.join(HERE, "depth_overlays_golden.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
