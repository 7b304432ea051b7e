#!/usr/bin/env python3
"""Golden vectors for the exclusive first-mask-wins labelling of a batch (lpf_first_match) -- made by executing the REFERENCE's own
source lines Same_color.py:114-132 (the validity filter and the per-point double loop, inline in the script's main loop) with
G.run_ref, the way make_golden_views.py does for frame 100.  The loop collects points and colours, not indices: it is given points
whose coordinates ARE their index and a palette whose colour i IS i, so both are read back from what it collected.

Inputs: every committed frame with its overlapping "edge" masks, and the constructed cases of tests/first_match_ref.py (masks smaller
and larger than the image, the float values around 0.5, a frame without masks, a frame without a valid point), which the tests
regenerate from the same seeds.  Only indices and mask ids are stored.

Usage: python tests/golden/make_golden_first_match.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as G  # noqa: E402
import first_match_ref as R  # noqa: E402


def same_color(points, masks, velo_to_rect, camera):
    """(car_idx, car_mask, bg_idx, n_valid) of one frame by the script's own lines"""
    ns = G.run_ref("V3_point_cloud_with_erosion.py", 565, 569, {"np": np, "points": points, "TrVeloToRect": velo_to_rect, "camera": camera},
                   "points_homo = points.copy()")
    tagged = np.repeat(np.arange(len(points), dtype=np.float64)[:, None], 4, axis=1)
    ns = G.run_ref("Same_color.py", 114, 132, {"np": np, "u": ns["u"], "v": ns["v"], "depth": ns["depth"], "camera": camera, "frame": 0,
                                                "points": tagged, "masks": list(masks), "mask_colors": [(i, i, i) for i in range(len(masks))]},
                   "valid = (u >= 0)")
    car = np.array([int(p[0]) for p in ns["colored_points"]], np.int32)
    mask = np.array([int(round(float(c[0]) * 255.0)) for c in ns["colored_colors"]], np.int16)
    bg = np.array([int(p[0]) for p in ns["full_points"]], np.int32)
    return car, mask, bg, len(ns["valid_indices"])


def main():
    G._seed_import_stubs()
    kitti360 = G.kitti360
    camera = kitti360.CameraPerspective(G.DATA, G.SEQ, 0)
    _, velo_to_rect = kitti360.velo_to_rect_transforms(G.DATA, camera, 0)
    calib = dict(np.load(os.path.join(HERE, "calib_cam0.npz")))
    assert np.array_equal(calib["TrVeloToRect"], velo_to_rect)
    with open(os.path.join(HERE, "index.json")) as f:
        frames = [r["frame"] for r in json.load(f)["frames"]]
    res = {"frames": np.array(frames, np.int64), "cases": np.array(R.CASES)}
    todo = [("f%d" % fr, R.golden_frame_case(dict(np.load(os.path.join(HERE, "frame_%010d.npz" % fr))), calib)) for fr in frames]
    todo += [(name, R.constructed_case(name, calib)) for name in R.CASES]
    for key, (points, masks) in todo:
        car, mask, bg, n_valid = same_color(points, masks, velo_to_rect, camera)
        assert n_valid == len(car) + len(bg)
        res[key + "_car"], res[key + "_mask"], res[key + "_bg"] = car, mask, bg
        print(key, "points", len(points), "masks", len(masks), "car", len(car), "background", len(bg))
    np.savez_compressed(os.path.join(HERE, "first_match_golden.npz"), **res)


if __name__ == "__main__":
    main()
