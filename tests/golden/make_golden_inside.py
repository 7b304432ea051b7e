#!/usr/bin/env python3
"""Golden vectors for V3's inside / outside split (lpf_inside_masks), made by running the REFERENCE's own V3
calculate_car_point_statistics (V3_point_cloud_with_erosion.py:320-428) in the build container on the committed frames
(tests/golden/frame_*.npz: their points, their instance lists and their velodyne-frame boxes), for the tags rect5_d50, rect5_d30 and
edge_d50, with use_oriented=True and use_oriented=False.  Same rules as make_golden.py: the module is imported in place behind inert
stubs, only inputs and outputs are written.

Per frame f, tag t and kind k in ("oriented", "aabb") (keys "<frame>_<tag>_<kind>_..."):
  car_id int64 [n], matched_bbox_id int64 [n]: the statistics dicts in order (cars without points have none)
  mask_off int64 [n + 1], mask_bits uint8: np.packbits of the dicts' inside_mask arrays, concatenated in order; an unmatched car
  (inside_mask None) has no bits
A frame without boxes (no box file, or no visible box) has no dicts: n = 0.

Usage: python tests/golden/make_golden_inside.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

TAGS = ("rect5_d50", "rect5_d30", "edge_d50")


def main():
    G._seed_import_stubs()
    v3 = G._load_ref("V3_point_cloud_with_erosion.py", "ref_v3i")
    frames = G.kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=G.DATA).available_frames()
    out = {"frames": np.array(frames, np.int64)}
    bits = matched = both = unmatched = empty = 0
    for frame in frames:
        g = dict(np.load(os.path.join(HERE, "frame_%010d.npz" % frame)))
        boxes3d = [{"corners_velo": c.tolist()} for c in g["corners_velo"]] if "corners_velo" in g else []
        for tag in TAGS:
            sets = []
            if "inst_count_" + tag in g:
                off = np.concatenate([[0], np.cumsum(g["inst_count_" + tag])])
                for a, b in zip(off[:-1], off[1:]):
                    sets.append(g["points"][g["inst_cat_" + tag][a:b], :3] if b > a else np.array([]).reshape(0, 3))
            colors = [(int(i * 60) % 255, int(i * 120) % 255, int(i * 180) % 255) for i in range(len(sets))]
            for kind, oriented in (("oriented", True), ("aabb", False)):
                stats = G._quiet(v3.calculate_car_point_statistics, sets, boxes3d, colors, min_points=10, use_oriented=oriented)
                masks = [np.asarray(s["inside_mask"], bool) if s["inside_mask"] is not None else np.zeros(0, bool) for s in stats]
                for s, m in zip(stats, masks):
                    assert s["inside_mask"] is None or len(m) == len(s["car_points"]) == s["total_points"]
                    assert int(m.sum()) == int(s["points_inside_bbox"])
                key = "%d_%s_%s_" % (frame, tag, kind)
                out[key + "car_id"] = np.array([s["car_id"] for s in stats], np.int64)
                out[key + "matched_bbox_id"] = np.array([s["matched_bbox_id"] for s in stats], np.int64)
                out[key + "mask_off"] = np.concatenate([[0], np.cumsum([len(m) for m in masks])]).astype(np.int64)
                out[key + "mask_bits"] = np.packbits(np.concatenate(masks) if masks else np.zeros(0, bool))
                if oriented:
                    bits += int(out[key + "mask_off"][-1])
                    matched += sum(s["matched_bbox_id"] >= 0 for s in stats)
                    both += sum(s["matched_bbox_id"] >= 0 and 0 < int(m.sum()) < len(m) for s, m in zip(stats, masks))
                    unmatched += sum(s["matched_bbox_id"] < 0 for s in stats)
                    empty += (sum(len(s) == 0 for s in sets) if boxes3d else 0)
    path = os.path.join(HERE, "inside_golden.npz")
    np.savez_compressed(path, **out)
    print("frames", len(frames), "oriented: mask bits", bits, "matched cars", matched, "with both parts", both, "unmatched", unmatched,
          "empty", empty, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
