#!/usr/bin/env python3
"""Golden vectors for the per-box point counts and first boxes (lpf_box_points), made by running the REFERENCE's own V3
oriented_point_in_bbox (V3_point_cloud_with_erosion.py:167-208) and point_in_bbox (V3:143-164) in the build container on
points_valid = points[valid_indices, :3] (V3:590-592) of the committed frames (tests/golden/frame_*.npz and the three *_full.npz:
their points and their velodyne-frame boxes), for both depth windows (d50, d30).  Same rules as make_golden.py: the module is imported
in place behind inert stubs, only inputs and outputs are written.  The valid indices are the committed ones (valid_idx_d50 / _d30);
the full-size frames and the frame without a box file store none, so theirs come from this project's restatement of V3:565-585
(tests/box_points_ref.py: valid_indices), which tests/test_box_points_api.py holds against the committed digests.

Per frame f ("<frame>" or "<frame>_full"), window w and kind k in ("oriented", "aabb") (keys "<f>_<w>_<k>_..."):
  box_sum  int32 [B]: np.sum of the reference's boolean array of each box
  first    int16 [n_valid]: the lowest box whose array holds the point, -1 if none
  two      int64: points held by at least two boxes
A frame without boxes (no box file, or no visible box) has B = 0 and every first = -1.

Usage: python tests/golden/make_golden_box_points.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import box_points_ref as R  # noqa: E402

FULL = (1461, 2098, 2449)


def main():
    G._seed_import_stubs()
    v3 = G._load_ref("V3_point_cloud_with_erosion.py", "ref_v3bp")
    fn = {"oriented": v3.oriented_point_in_bbox, "aabb": v3.point_in_bbox}
    cal = dict(np.load(os.path.join(HERE, "calib_cam0.npz")))
    T, K3, W, H = cal["TrVeloToRect"], cal["K"][:3, :3], int(cal["width"]), int(cal["height"])
    frames = G.kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=G.DATA).available_frames()
    out = {"frames": np.array(frames, np.int64), "full_frames": np.array(FULL, np.int64)}
    tot = dict(valid=0, boxes=0, empty=0, boxed=0, two=0, largest=0)
    for name, sub in [("%d" % f, True) for f in frames] + [("%d_full" % f, False) for f in FULL]:
        g = dict(np.load(os.path.join(HERE, "frame_%010d%s.npz" % (int(name.split("_")[0]), "" if sub else "_full"))))
        corners = g["corners_velo"] if "corners_velo" in g else np.zeros((0, 8, 3))
        for win, dmax in R.WINDOWS:
            vi = g["valid_idx_" + win] if ("valid_idx_" + win) in g else R.valid_indices(g["points"], T, K3, W, H, dmax)
            points_valid = g["points"][vi, :3]
            for kind, _ in R.KINDS:
                inside = np.zeros((len(corners), len(vi)), bool)
                for b, c in enumerate(corners):
                    inside[b] = fn[kind](points_valid, c)
                key = "%s_%s_%s_" % (name, win, kind)
                per_point = inside.sum(axis=0)
                out[key + "box_sum"] = inside.sum(axis=1).astype(np.int32)
                first = np.where(per_point > 0, inside.argmax(axis=0), -1) if len(corners) else np.full(len(vi), -1)
                assert len(corners) < 32767
                out[key + "first"] = first.astype(np.int16)
                out[key + "two"] = np.int64((per_point >= 2).sum())
                if sub and win == "d50" and kind == "oriented" and len(corners):
                    tot["valid"] += len(vi); tot["boxes"] += len(corners); tot["empty"] += int((out[key + "box_sum"] == 0).sum())
                    tot["boxed"] += int((per_point > 0).sum()); tot["two"] += int((per_point >= 2).sum())
                    tot["largest"] = max(tot["largest"], int(out[key + "box_sum"].max()))
    path = os.path.join(HERE, "box_points_golden.npz")
    np.savez_compressed(path, **out)
    print("oriented d50, sub-sampled frames with boxes:", tot, "bytes", os.path.getsize(path))
    assert tot == dict(valid=53843, boxes=472, empty=304, boxed=7077, two=681, largest=2945), tot


if __name__ == "__main__":
    main()
