#!/usr/bin/env python3
"""Golden vectors for the batched box-view filter and box projection (lpf_box_views), made by running the REFERENCE's own functions in
the build container: secondtest.py's is_bbox_in_camera_view and filter_bboxes_in_camera_view and V5_ProjectingBBoxes.py's
project_3d_bbox_to_2d.  Same rules as make_golden.py: the modules are imported in place behind inert stubs, only inputs and outputs
are written.

Three sets of boxes (keys "<set>_..."):
  a  the sample: every box of every box file, frame by frame, under the sample camera
  b  SEEDED boxes under the sample camera (tests/box_views_ref.py: seeded_boxes(N_SEEDED, 0)): centre x U(-60,60), y U(-2,3),
     z U(-20,140), extent (1.65, 1.97, 4.43) * U(0.05, 1.2), every corner the centre +- half the extent with random signs; in frames
     of PER_FRAME
  c  border cases under a second camera, K = [[512,0,640],[0,512,188],[0,0,1]], 1280 x 376, so that ties and borders are exact: pixel
     ties at k + 0.5 for both parities of k; u and v at -1, 0, W - 1 and W (H - 1 and H); depth at exactly 0.1, 100 and 0 and just
     outside 0.1 and 100; area at exactly 99 and 100; 3 and 4 corners in view; every count 0..8 of near corners and of front corners
Per set: corners float64 [B,8,3], box_off int64 [F+1], and every field the functions return (absent ones -1 / NaN):
  keep, reason (index into REASONS), corners_in_view, corners_near (corners_with_valid_depth), avg_depth, depths [B,8]
  (all_behind_camera), bbox_2d [B,4] (no_intersection), small [B,3] = projected_area, u_range, v_range (too_small)
  proj_ok, proj_bbox, proj_center, proj_size, proj_area, proj_avg_depth (project_3d_bbox_to_2d)
  kept_count int64 [F], filter_reasons (one repr of stats['filter_reasons'] per line and frame), stdout (filter_bboxes_in_camera_view's
  printed lines, verbose, all frames)
"c_K", "c_size": the second camera.

Usage: python tests/golden/make_golden_box_views.py
"""
import contextlib
import copy
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402
import box_views_ref as R  # noqa: E402

N_SEEDED = 1500
PER_FRAME = 125
K2 = np.array([[512.0, 0.0, 640.0], [0.0, 512.0, 188.0], [0.0, 0.0, 1.0]])
W2, H2 = 1280, 376


def box_at(uvz):
    """a box whose corner i projects to pixel (u, v) at depth z under K2 (exactly, for z a power of two): uvz is 8 x (u, v, z)"""
    uvz = np.asarray(uvz, np.float64).reshape(8, 3)
    z = uvz[:, 2]
    zz = np.where(z == 0, 1.0, z)                            # (a corner at depth 0: x and y as at depth 1)
    return np.stack([(uvz[:, 0] - K2[0, 2]) * zz / K2[0, 0], (uvz[:, 1] - K2[1, 2]) * zz / K2[1, 1], z], axis=1)


def border_cases():
    rect = lambda x0, y0, x1, y1, z=1.0: [(x0, y0, z), (x1, y0, z), (x0, y1, z), (x1, y1, z)] * 2
    out = []
    # pixel ties at k + 0.5, both parities (half to even): 10.5 -> 10, 11.5 -> 12, and on the image's borders
    for a in (10.5, 11.5, -0.5, 0.5, W2 - 1.5, W2 - 0.5):
        out.append(box_at(rect(a, 20.5, a + 40.0, 61.5)))
        out.append(box_at(rect(100.0, min(a, H2 - 0.5), 160.0, min(a, H2 - 0.5) + 30.0)))
    for b in (-0.5, 0.5, H2 - 1.5, H2 - 0.5):
        out.append(box_at(rect(300.5, b, 341.5, b + 25.0)))
    # u and v at -1, 0, W - 1, W (H - 1, H): boxes that end / begin exactly there
    for x1 in (-1, 0):
        out.append(box_at(rect(x1 - 50, 100, x1, 150)))     # ends at -1: misses; at 0: touches
    for x0 in (W2 - 1, W2):
        out.append(box_at(rect(x0, 100, x0 + 50, 150)))
    for y1 in (-1, 0):
        out.append(box_at(rect(500, y1 - 50, 560, y1)))
    for y0 in (H2 - 1, H2):
        out.append(box_at(rect(500, y0, 560, y0 + 50)))
    # depth at exactly 0.1, 100 and 0, and just outside 0.1 and 100: all eight corners, then one corner
    for z in (0.1, np.nextafter(0.1, 0.0), 100.0, np.nextafter(100.0, np.inf), 0.0):
        out.append(box_at(rect(600, 150, 700, 250, z)))
        c = rect(600, 150, 700, 250)
        c[3] = (700, 250, z)
        out.append(box_at(c))
        c = rect(600, 150, 700, 250, 200.0)                  # seven in front but too far, one at z
        c[5] = (650, 200, z)
        out.append(box_at(c))
    # area at exactly 99 and 100 (and around)
    for w, h in ((9, 11), (11, 9), (10, 10), (99, 1), (100, 1), (1, 100), (33, 3), (0, 500), (500, 0), (50, 2), (49, 2)):
        out.append(box_at(rect(400, 100, 400 + w, 100 + h)))
    # 3 and 4 corners in view, the others beside the image; then the same with the pixel box missing the image (no corner in view)
    for n in (0, 1, 2, 3, 4, 5):
        c = [(200 + 30 * i, 100 + 20 * (i % 2), 1.0) for i in range(8)]
        for i in range(n, 8):
            c[i] = (W2 + 10 + 30 * i, 100 + 20 * (i % 2), 1.0)
        out.append(box_at(c))
    for n in (1, 3, 4):                                      # few near corners, all beside the image: no_intersection
        c = [(-500 - 30 * i, 100 + 20 * (i % 2), 1.0 if i < n else -1.0) for i in range(8)]
        out.append(box_at(c))
        c = [(200 + 30 * i, H2 + 5 + 20 * (i % 2), 1.0 if i < n else 400.0) for i in range(8)]
        out.append(box_at(c))
    # every count 0..8 of near corners and of front corners: the others behind the camera, or in front but too far
    for n in range(9):
        for other in (-1.0, 256.0, -0.0625):
            c = [(200 + 40 * i, 60 + 30 * (i % 3), 1.0 if i < n else other) for i in range(8)]
            out.append(box_at(c))
            c = [(200 + 40 * i, 60 + 30 * (i % 3), 1.0 if i >= 8 - n else other) for i in range(8)]     # the near ones last
            out.append(box_at(c))
    return np.array(out, np.float64).reshape(-1, 8, 3)


def run_set(second, v5, camera, boxes_per_frame):
    boxes = [b for fr in boxes_per_frame for b in fr]
    o = R.scalar_fields(boxes, camera, second.is_bbox_in_camera_view, v5.project_3d_bbox_to_2d)
    o["corners"] = np.array([b["corners_cam0"] for b in boxes], np.float64).reshape(-1, 8, 3)
    o["box_off"] = np.concatenate([[0], np.cumsum([len(fr) for fr in boxes_per_frame])]).astype(np.int64)
    kept_count, reasons = [], []
    buf = io.StringIO()
    for fr, a, b in zip(boxes_per_frame, o["box_off"][:-1], o["box_off"][1:]):
        with contextlib.redirect_stdout(buf):
            kept, stats = second.filter_bboxes_in_camera_view(fr, camera, True)
        assert [x["index"] for x in kept] == [x["index"] for x, k in zip(fr, o["keep"][a:b]) if k]
        assert stats["total"] == len(fr) and stats["kept"] == len(kept)
        kept_count.append(stats["kept"])
        reasons.append(repr(stats["filter_reasons"]))
    o["kept_count"], o["filter_reasons"], o["stdout"] = np.array(kept_count, np.int64), np.array("\n".join(reasons)), np.array(buf.getvalue())
    return o


def as_dicts(corners, per_frame):
    boxes = [{"index": i, "corners_cam0": c.tolist()} for i, c in enumerate(corners)]
    return [boxes[i:i + per_frame] for i in range(0, len(boxes), per_frame)]


def main():
    G._seed_import_stubs()
    second = G._load_ref("secondtest.py", "ref_second_bv")
    v5 = G._load_ref("V5_ProjectingBBoxes.py", "ref_v5_bv")
    v3 = G._load_ref("V3_point_cloud_with_erosion.py", "ref_v3_bv")
    kitti360 = G.kitti360
    camera = kitti360.CameraPerspective(G.DATA, G.SEQ, 0)
    frames = kitti360.Kitti360Viewer3DRaw(seq=0, root_dir=G.DATA).available_frames()
    sample, sample_frames = [], []
    for frame in frames:
        raw = G._quiet(v3.load_bounding_boxes, os.path.join(G.DATA, "bboxes_3D_cam0", "BBoxes_%d.json" % frame))
        if raw:
            sample.append(raw)
            sample_frames.append(frame)
    camera2 = copy.copy(camera)
    camera2.K = np.eye(4)
    camera2.K[:3, :3] = K2
    camera2.width, camera2.height = W2, H2
    sets = {"a": run_set(second, v5, camera, sample),
            "b": run_set(second, v5, camera, as_dicts(R.seeded_boxes(N_SEEDED, 0), PER_FRAME)),
            "c": run_set(second, v5, camera2, as_dicts(border_cases(), 1 << 30))}
    out = {"a_frames": np.array(sample_frames, np.int64), "c_K": K2, "c_size": np.array([W2, H2], np.int64)}
    for name, o in sets.items():
        cam = camera2 if name == "c" else camera
        u, v, d = R.project(o["corners"], cam.K)
        assert np.abs(u).max() < 2 ** 31 and np.abs(v).max() < 2 ** 31, name         # the library's pixels are these integers as float64
        assert np.isfinite(o["corners"]).all()
        if name != "a":
            counts = np.bincount(o["reason"], minlength=6)
            assert all(counts[r] > 0 for r in (0, 2, 3, 4)), (name, counts)
            near = ((d >= 0.1) & (d <= 100)).sum(axis=1)
            front = (d > 0).sum(axis=1)
            assert set(near.tolist()) == set(range(9)) and set(front.tolist()) == set(range(9)), name
        for k, a in o.items():
            out["%s_%s" % (name, k)] = a
        print(name, "boxes", len(o["keep"]), "frames", len(o["box_off"]) - 1, "reasons", np.bincount(o["reason"], minlength=6).tolist())
    path = os.path.join(HERE, "box_views_golden.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
