#!/usr/bin/env python3
"""Golden vectors for the 2D detection-to-box matching (lpf_match_2d), made by running the REFERENCE's own functions in the build
container: V4_BBox_IoU_filtering.py's calculate_iou_2d and match_detections_to_bboxes, V5_ProjectingBBoxes.py's
project_3d_bbox_to_2d, calculate_matching_score and improved_match_detections_to_bboxes, on every box file of the sample.  Same rules
as make_golden.py: the modules are imported in place behind inert stubs, only inputs and outputs are written.

Detections (float32, as the detector's boxes.xyxy) come from a seeded rule: the projections of up to DETS_FROM_BOXES boxes of the frame
that reach into the image, clipped to it and jittered by a few pixels (fractions included), plus UNRELATED boxes placed at random.

Per frame f (keys "<frame>_..."):
  dets float32 [D,4]; bbox2d int64 [B,4] and front int64 [B] (the reference's projection of every box, front = corners with depth > 0)
  iou / center / size / total / cost float64 [D,B] from calculate_iou_2d / calculate_matching_score per pair -- columns of boxes
  without a projection are 0 (cost 1) -- for frames with D * B <= FULL_OVER, else their SHA-256 ("<name>_sha")
  v4_corners [n,8,3], v4_colors [n,3]: match_detections_to_bboxes' list;  v4_best int64 [D]: the box each detection chose (-1: none)
  v5_rows, v5_cols: linear_sum_assignment of the cost matrix without the columns that have no projection
  v5_corners [n,8,3], v5_colors [n,3], v5_stdout: improved_match_detections_to_bboxes' list and printed lines
The reference scores np.int64 pixels, the library the same values as float64: they agree while a rectangle's area stays below 2^53,
which is asserted here.

Usage: python tests/golden/make_golden_match2d.py
"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402

SEED = 20261016
DETS_FROM_BOXES = 10
UNRELATED = 2
FULL_OVER = 1024                  # matrices with more elements are stored as their SHA-256


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def detections(rng, rects, front, W, H):
    """the seeded rule: float32 [D,4]"""
    inside = [j for j in range(len(rects)) if front[j] > 0 and rects[j][0] < W and rects[j][2] > 0 and rects[j][1] < H and rects[j][3] > 0
              and rects[j][2] > rects[j][0] and rects[j][3] > rects[j][1]]
    pick = sorted(rng.choice(inside, size=min(DETS_FROM_BOXES, len(inside)), replace=False).tolist()) if inside else []
    dets = []
    for j in pick:
        x0, y0, x1, y1 = (float(v) for v in rects[j])
        x0, x1, y0, y1 = max(x0, 0.0), min(x1, W - 1.0), max(y0, 0.0), min(y1, H - 1.0)
        if j % 4 == 0:                                        # every fourth one exactly on its (clipped) box
            dets.append([x0, y0, x1, y1])
        else:
            jit = rng.normal(0.0, 4.0, 4)
            dets.append([x0 + jit[0], y0 + jit[1], x1 + jit[2], y1 + jit[3]])
    for _ in range(UNRELATED):
        a, b = rng.uniform(0, W - 60), rng.uniform(0, H - 40)
        dets.append([a, b, a + rng.uniform(10, 300), b + rng.uniform(10, 150)])
    return np.array(dets, np.float32).reshape(-1, 4)


def main():
    G._seed_import_stubs()
    v4 = G._load_ref("V4_BBox_IoU_filtering.py", "ref_v4m")
    v5 = G._load_ref("V5_ProjectingBBoxes.py", "ref_v5m")
    from scipy.optimize import linear_sum_assignment
    kitti360 = G.kitti360
    camera = kitti360.CameraPerspective(G.DATA, G.SEQ, 0)
    velo_to_cam, _ = kitti360.velo_to_rect_transforms(G.DATA, camera, 0)
    frames = kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=G.DATA).available_frames()
    W, H = camera.width, camera.height
    out = {"frames": [], "seed": np.int64(SEED)}
    n_pairs = n_overlap = 0
    largest = 0
    for frame in frames:
        raw = G._quiet(v4.load_bounding_boxes, os.path.join(G.DATA, "bboxes_3D_cam0", "BBoxes_%d.json" % frame))
        if not raw:
            continue
        boxes = G._quiet(v5.transform_bboxes_to_velodyne, [dict(b) for b in raw], velo_to_cam)
        infos = [G._quiet(v5.project_3d_bbox_to_2d, b, camera)[0] for b in boxes]
        B = len(boxes)
        rects, front = np.zeros((B, 4), np.int64), np.zeros(B, np.int64)
        for j, (b, info) in enumerate(zip(boxes, infos)):
            front[j] = int((camera.cam2image(np.array(b["corners_cam0"]).T)[2] > 0).sum())
            assert (info is not None) == (front[j] > 0)
            if info is not None:
                rects[j] = info["bbox"]
                assert all(isinstance(v, np.integer) for v in info["bbox"])
                largest = max(largest, abs(int(info["area"])), int(np.abs(rects[j]).max()))
        assert largest < 2 ** 53
        rng = np.random.default_rng(SEED + frame)
        dets = detections(rng, rects, front, W, H)
        D = len(dets)
        colors = v5.generate_consistent_colors(max(D - 1, 0))          # one colour short: V5's red fallback for the last detection
        colors4 = v5.generate_consistent_colors(D)
        m = {k: np.zeros((D, B)) for k in ("iou", "center", "size", "total", "cost")}
        m["cost"][:] = 1.0
        det_infos = []
        for box in dets:
            x1, y1, x2, y2 = box
            det_infos.append({"bbox": [x1, y1, x2, y2], "center": [(x1 + x2) / 2, (y1 + y2) / 2], "size": [x2 - x1, y2 - y1],
                              "area": (x2 - x1) * (y2 - y1)})                  # V5:324-330
        for i in range(D):
            for j, info in enumerate(infos):
                if info is None:
                    continue
                score, det = v5.calculate_matching_score(det_infos[i], info)
                x1, y1, x2, y2 = dets[i]
                assert det["iou"] == v4.calculate_iou_2d([x1, y1, x2, y2], info["bbox"])
                m["iou"][i, j], m["center"][i, j], m["size"][i, j], m["total"][i, j] = det["iou"], det["center_score"], det["size_score"], score
                m["cost"][i, j] = 1 - score
        n_pairs += D * B
        n_overlap += int((m["iou"] > 0).sum())
        key = "%d_" % frame
        out["frames"].append(frame)
        out[key + "dets"], out[key + "bbox2d"], out[key + "front"] = dets, rects, front
        for k, a in m.items():
            if D * B <= FULL_OVER:
                out[key + k] = a
            else:
                out[key + k + "_sha"] = np.array(sha(a))
        pairs = G._quiet(v4.match_detections_to_bboxes, dets, boxes, colors4, camera)
        out[key + "v4_corners"] = np.array([p[0] for p in pairs], np.float64).reshape(-1, 8, 3)
        out[key + "v4_colors"] = np.array([p[1] for p in pairs], np.float64).reshape(-1, 3)
        best = np.full(D, -1, np.int64)                     # the box behind each pair: V4 appends pairs in detection order
        cv = np.array([b["corners_velo"] for b in boxes], np.float64).reshape(-1, 8, 3)
        k = 0
        for i in range(D):
            row = m["iou"][i]
            j = int(np.argmax(row)) if B else -1
            if B and row[j] > 0.25:
                assert np.array_equal(out[key + "v4_corners"][k], cv[j]), (frame, i)
                best[i] = j
                k += 1
        assert k == len(pairs)
        out[key + "v4_best"] = best
        valid = np.flatnonzero(front > 0)
        rows, cols = linear_sum_assignment(m["cost"][:, valid]) if len(valid) and D else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        out[key + "v5_rows"], out[key + "v5_cols"] = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            pairs5 = v5.improved_match_detections_to_bboxes(dets, boxes, colors, camera)
        out[key + "v5_corners"] = np.array([p[0] for p in pairs5], np.float64).reshape(-1, 8, 3)
        out[key + "v5_colors"] = np.array([p[1] for p in pairs5], np.float64).reshape(-1, 3)
        out[key + "v5_stdout"] = np.array(buf.getvalue())
    out["frames"] = np.array(out["frames"], np.int64)
    path = os.path.join(HERE, "match2d_golden.npz")
    np.savez_compressed(path, **out)
    print("frames", len(out["frames"]), "pairs", n_pairs, "with IoU > 0", n_overlap, "largest coordinate / area", largest,
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
