#!/usr/bin/env python3
"""Golden vectors for the Hungarian assignment on the GPU (lpf_assign_costs, lpf_assign_2d), made in the build container:

1. the seeded case list of tests/assign_ref.py with scipy.optimize.linear_sum_assignment's answers ("case_<name>_rows" / "_cols";
   the matrix itself, "case_<name>", for cases of up to STORE_OVER elements, else its SHA-256 "case_<name>_sha": the list is
   regenerated from its seed and checked against these);
2. the REFERENCE's own improved_match_detections_to_bboxes (V5_ProjectingBBoxes.py:307-416), imported in place behind inert stubs as
   make_golden_match2d.py does, on every box file of the sample with 5, 32 and 256 seeded float32 detections per frame.  Per frame f
   and count n (keys "<frame>_<n>_..."): dets float32 [n,4]; rows, cols: what the function's linear_sum_assignment call returned
   (cols are compact: ranks among the boxes with a projection); v5_box int32 [m]: the box behind each entry of the returned list;
   v5_colors float64 [m,3]; v5_stdout: the printed lines.

Detections come from a seeded rule: three of four are the (clipped) projection of a random box of the frame that reaches into the
image -- every fourth of those exactly, the others jittered by a few pixels -- the rest are placed at random.  With more detections
than boxes many rows repeat, so the cost matrix ties as V5's does.

Usage: python tests/golden/make_golden_assign.py
"""
import contextlib
import hashlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import assign_ref as A  # noqa: E402
import make_golden as G  # noqa: E402

SEED = 20261019
COUNTS = (5, 32, 256)
STORE_OVER = 64 * 65              # matrices with more elements are stored as their SHA-256


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float64).tobytes()).hexdigest()


def detections(rng, n, rects, front, W, H):
    """the seeded rule: float32 [n,4]"""
    inside = [j for j in range(len(rects)) if front[j] > 0 and rects[j][0] < W and rects[j][2] > 0 and rects[j][1] < H and rects[j][3] > 0
              and rects[j][2] > rects[j][0] and rects[j][3] > rects[j][1]]
    dets = []
    for i in range(n):
        if inside and i % 4 != 3:
            j = inside[int(rng.integers(len(inside)))]
            x0, y0, x1, y1 = (float(v) for v in rects[j])
            x0, x1, y0, y1 = max(x0, 0.0), min(x1, W - 1.0), max(y0, 0.0), min(y1, H - 1.0)
            jit = rng.normal(0.0, 4.0, 4) if i % 4 else np.zeros(4)
            dets.append([x0 + jit[0], y0 + jit[1], x1 + jit[2], y1 + jit[3]])
        else:
            a, b = rng.uniform(0, W - 60), rng.uniform(0, H - 40)
            dets.append([a, b, a + rng.uniform(10, 300), b + rng.uniform(10, 150)])
    return np.array(dets, np.float32).reshape(-1, 4)


def main():
    from scipy.optimize import linear_sum_assignment
    out = {"seed": np.int64(SEED), "counts": np.array(COUNTS, np.int64)}
    names = []
    for name, m in A.cases():
        rows, cols = linear_sum_assignment(m)
        st, r, c = A.solve(m)
        assert st == 0 and np.array_equal(r, rows) and np.array_equal(c, cols), name
        names.append(name)
        if m.size <= STORE_OVER:
            out["case_" + name] = m
        else:
            out["case_" + name + "_sha"] = np.array(sha(m))
        out["case_" + name + "_rows"], out["case_" + name + "_cols"] = rows.astype(np.int32), cols.astype(np.int32)
    out["case_names"] = np.array(names)

    G._seed_import_stubs()
    v4 = G._load_ref("V4_BBox_IoU_filtering.py", "ref_v4a")
    v5 = G._load_ref("V5_ProjectingBBoxes.py", "ref_v5a")
    calls = []

    def recording(cost):
        rows, cols = linear_sum_assignment(cost)
        calls.append((np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.array(cost).shape))
        return rows, cols
    assert hasattr(v5, "linear_sum_assignment")
    v5.linear_sum_assignment = recording                      # (the module's own name for scipy's function: its calls are recorded)
    kitti360 = G.kitti360
    camera = kitti360.CameraPerspective(G.DATA, G.SEQ, 0)
    velo_to_cam, _ = kitti360.velo_to_rect_transforms(G.DATA, camera, 0)
    frames = kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=G.DATA).available_frames()
    W, H = camera.width, camera.height
    done = []
    for frame in frames:
        raw = G._quiet(v4.load_bounding_boxes, os.path.join(G.DATA, "bboxes_3D_cam0", "BBoxes_%d.json" % frame))
        if not raw:
            continue
        boxes = G._quiet(v5.transform_bboxes_to_velodyne, [dict(b) for b in raw], velo_to_cam)
        B = len(boxes)
        rects, front = np.zeros((B, 4), np.int64), np.zeros(B, np.int64)
        for j, b in enumerate(boxes):
            info = G._quiet(v5.project_3d_bbox_to_2d, b, camera)[0]
            front[j] = int((camera.cam2image(np.array(b["corners_cam0"]).T)[2] > 0).sum())
            if info is not None:
                rects[j] = info["bbox"]
        cv = np.array([b["corners_velo"] for b in boxes], np.float64).reshape(-1, 8, 3)
        done.append(frame)
        for n in COUNTS:
            rng = np.random.default_rng(SEED + 1000 * frame + n)
            dets = detections(rng, n, rects, front, W, H)
            colors = v5.generate_consistent_colors(max(n - 1, 0))      # one colour short: V5's red fallback for the last detection
            del calls[:]
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                pairs = v5.improved_match_detections_to_bboxes(dets, boxes, colors, camera)
            if not calls:                                    # the function left before it assigned (no box with a projection)
                assert not (front > 0).any(), (frame, n)
                calls.append((np.zeros(0, np.int64), np.zeros(0, np.int64), (n, 0)))
            assert len(calls) == 1 and calls[0][2] == (n, int((front > 0).sum())), (frame, n, calls)
            which = []                                       # (boxes with equal corners: the first one not yet listed; the lists are the same)
            for corners, _ in pairs:
                hit = [int(j) for j in np.flatnonzero((cv == np.asarray(corners)).all(axis=(1, 2))) if int(j) not in which]
                assert hit, (frame, n)
                which.append(hit[0])
            key = "%d_%d_" % (frame, n)
            out[key + "dets"] = dets
            out[key + "rows"], out[key + "cols"] = calls[0][0].astype(np.int32), calls[0][1].astype(np.int32)
            out[key + "v5_box"] = np.array(which, np.int32)
            out[key + "v5_colors"] = np.array([p[1] for p in pairs], np.float64).reshape(-1, 3)
            out[key + "v5_stdout"] = np.array(buf.getvalue())
    out["frames"] = np.array(done, np.int64)
    path = os.path.join(HERE, "assign_golden.npz")
    np.savez_compressed(path, **out)
    print("cases", len(names), "frames", len(done), "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
