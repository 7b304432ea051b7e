"""A vectorised NumPy restatement of lpf_box_views (include/lpf.h): secondtest.py's is_bbox_in_camera_view and V5's detailed
project_3d_bbox_to_2d for every box of a batch, with the rank of the kept boxes and the counts per reason.  tests/test_box_views_api.py
holds it against the scalar functions of the package and against goldens made by the reference's own functions
(tests/golden/make_golden_box_views.py); tests/test_gpu_box_views.py holds the GPU against it, bit for bit."""
import contextlib
import io

import numpy as np

REASONS = ("valid", "no_corners", "all_behind_camera", "no_intersection", "too_small", "error")
WANT = ("keep", "reason", "corners_in_view", "corners_near", "avg_depth", "near_bbox2d", "front", "bbox2d", "front_avg_depth",
        "kept_pos", "frame_counts", "corners_velo")
BIG = 1e300                       # what an empty corner set leaves in its pixel box: {BIG, BIG, -BIG, -BIG}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def project(corners, K3):
    """cam2image's statements on [B,8,3] corners: (u, v) as float64 (the integers np.round gives) and the depth, [B,8] each"""
    pts = np.asarray(corners, np.float64).reshape(-1, 8, 3).transpose(0, 2, 1)           # a box's corners.T, as the reference passes them
    proj = np.matmul(np.asarray(K3, np.float64)[:3, :3].reshape(1, 3, 3), pts)
    depth = proj[:, 2, :]
    depth[depth == 0] = -1e-6
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = np.round(proj[:, 0, :] / np.abs(depth))
        v = np.round(proj[:, 1, :] / np.abs(depth))
    return u, v, depth.copy()


def mean_in_numpy_order(d, m):
    """np.mean(d[b][m[b]]) per row: fewer than 8 values are summed left to right from 0.0, exactly 8 pairwise
    ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); one division by the count; 0.0 for an empty set"""
    s = np.zeros(len(d))
    for k in range(8):
        s = np.where(m[:, k], s + d[:, k], s)
    pair = ((d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3])) + ((d[:, 4] + d[:, 5]) + (d[:, 6] + d[:, 7]))
    n = m.sum(axis=1)
    s = np.where(n == 8, pair, s)
    return np.where(n > 0, s / np.maximum(n, 1), 0.0)


def pixel_box(u, v, m):
    """{min u, min v, max u, max v} over the corners of m, float64 [B,4]; the sentinels where m has none.  The reference's pixels are
    integers; as float64 a rounded pixel may be -0.0, and the zeros are ordered as include/lpf.h states it (-0 < +0: IEEE 754-2019's
    minimum and maximum, where NumPy's min / max keep whichever zero they meet first)."""
    def lo(a):
        w = np.where(m, a, BIG)
        r = w.min(axis=1)
        return np.where(r == 0, np.where(((w == 0) & np.signbit(w)).any(axis=1), -0.0, 0.0), r)

    def hi(a):
        w = np.where(m, a, -BIG)
        r = w.max(axis=1)
        return np.where(r == 0, np.where(((w == 0) & ~np.signbit(w)).any(axis=1), 0.0, -0.0), r)
    return np.stack([lo(u), lo(v), hi(u), hi(v)], axis=1)


def corners_velo(corners, T_cam_to_velo):
    """transform_bboxes_to_velodyne's statement, box by box (V3:41-52)"""
    T = np.asarray(T_cam_to_velo, np.float64).reshape(4, 4)
    out = np.zeros((len(corners), 8, 3))
    for i, c in enumerate(corners):
        homo = np.hstack([c, np.ones((8, 1))])
        out[i] = np.matmul(T, homo.T).T[:, :3]
    return out


def views(corners, box_off, K3, W, H, T_cam_to_velo=None, min_points_in_view=4, depth_range=(0.1, 100), min_area=100, want=WANT):
    """every output of lpf_box_views as the dict LpfContext.box_views returns"""
    corners = np.ascontiguousarray(corners, np.float64).reshape(-1, 8, 3)
    box_off = np.asarray(box_off, np.int64)
    B, F = len(corners), len(box_off) - 1
    u, v, d = project(corners, K3)
    near = (d >= depth_range[0]) & (d <= depth_range[1])
    n_near = near.sum(axis=1)
    in_view = (near & (u >= 0) & (u < W) & (v >= 0) & (v < H)).sum(axis=1)
    nb = pixel_box(u, v, near)
    x0, y0, x1, y1 = nb.T
    reason = np.zeros(B, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        small = (n_near >= 2) & ((x1 - x0) * (y1 - y0) < min_area)
    miss = (in_view < min_points_in_view) & ((x1 < 0) | (x0 >= W) | (y1 < 0) | (y0 >= H))
    reason[small] = 4
    reason[miss] = 3                                         # (the reference asks this before the size)
    reason[n_near == 0] = 2
    keep = reason == 0
    front = d > 0
    kept_pos = np.full(B, -1, np.int32)
    counts = np.zeros((F, 6), np.int32)
    for f in range(F):
        a, b = box_off[f], box_off[f + 1]
        k = keep[a:b]
        kept_pos[a:b][k] = np.arange(int(k.sum()), dtype=np.int32)
        counts[f] = np.bincount(reason[a:b], minlength=6)
    res = {"keep": keep.astype(np.uint8), "reason": reason, "corners_in_view": in_view.astype(np.int32),
           "corners_near": n_near.astype(np.int32), "avg_depth": mean_in_numpy_order(d, near), "near_bbox2d": nb,
           "front": front.sum(axis=1).astype(np.int32), "bbox2d": pixel_box(u, v, front),
           "front_avg_depth": mean_in_numpy_order(d, front), "kept_pos": kept_pos, "frame_counts": counts}
    if "corners_velo" in want:
        res["corners_velo"] = corners_velo(corners, T_cam_to_velo)
    return {w: res[w] for w in want}


class RefContext:
    """a context whose box_views is the restatement: what the batched pipeline functions see of the GPU (its match_2d: match2d_ref's)"""
    def __init__(self, K3, W, H):
        self.K3, self.W, self.H = np.asarray(K3, np.float64)[:3, :3], W, H
        self.calls = {"box_views": 0, "match_2d": 0}

    def ensure_intrinsics(self, K, width, height):
        assert np.array_equal(np.asarray(K, np.float64)[:3, :3], self.K3) and (width, height) == (self.W, self.H)

    def box_views(self, corners, box_off, T_cam_to_velo=None, min_points_in_view=4, depth_range=(0.1, 100), min_area=100,
                  want=("keep", "reason")):
        from lidar_object_detection_amd._native import LpfContext
        self.calls["box_views"] += 1
        LpfContext.box_views_batch(corners, box_off, T_cam_to_velo, min_points_in_view, depth_range, min_area, want)
        return views(corners, box_off, self.K3, self.W, self.H, T_cam_to_velo, min_points_in_view, depth_range, min_area, tuple(want))

    def match_2d(self, dets, bbox2d, front, min_iou=0.25, weights=(0.5, 0.3, 0.2), want=("best",)):
        import match2d_ref
        from lidar_object_detection_amd._native import LpfContext
        self.calls["match_2d"] += 1
        LpfContext.match2d_batch(dets, bbox2d, front)
        res = {}
        for d, b, f in zip(dets, bbox2d, front):
            m = match2d_ref.match(d, b, f, min_iou, weights)
            for k in (("best_box", "best_iou") if "best" in want else ()) + tuple(w for w in want if w != "best"):
                res.setdefault(k, []).append(m[k])
        return res


# ---- the scalar functions, box by box, packed as the goldens are (tests/golden/make_golden_box_views.py) ------------------------------
def scalar_fields(boxes, camera, is_in_view, project_box):
    """is_bbox_in_camera_view and project_3d_bbox_to_2d on every box dict: every returned field as arrays (absent: -1 / NaN)"""
    B = len(boxes)
    o = {"keep": np.zeros(B, bool), "reason": np.zeros(B, np.int8), "corners_in_view": np.full(B, -1, np.int64),
         "corners_near": np.full(B, -1, np.int64), "avg_depth": np.full(B, np.nan), "depths": np.full((B, 8), np.nan),
         "bbox_2d": np.zeros((B, 4), np.int64), "small": np.zeros((B, 3), np.int64),
         "proj_ok": np.zeros(B, bool), "proj_bbox": np.zeros((B, 4), np.int64), "proj_center": np.zeros((B, 2)),
         "proj_size": np.zeros((B, 2), np.int64), "proj_area": np.zeros(B, np.int64), "proj_avg_depth": np.full(B, np.nan)}
    for i, b in enumerate(boxes):
        ok, info = is_in_view(b, camera)
        o["keep"][i], o["reason"][i] = bool(ok), REASONS.index(info["reason"])
        o["corners_in_view"][i] = int(info.get("corners_in_view", -1))
        o["corners_near"][i] = int(info.get("corners_with_valid_depth", -1))
        o["avg_depth"][i] = float(info.get("avg_depth", np.nan))
        if "depths" in info:
            o["depths"][i] = info["depths"]
        if "bbox_2d" in info:
            o["bbox_2d"][i] = [int(x) for x in info["bbox_2d"]]
        if "projected_area" in info:
            o["small"][i] = [int(info["projected_area"]), int(info["u_range"]), int(info["v_range"])]
        with contextlib.redirect_stdout(io.StringIO()):
            pi, _ = project_box(b, camera)
        if pi is not None:
            o["proj_ok"][i] = True
            o["proj_bbox"][i], o["proj_center"][i], o["proj_size"][i] = [int(x) for x in pi["bbox"]], pi["center"], [int(x) for x in pi["size"]]
            o["proj_area"][i], o["proj_avg_depth"][i] = int(pi["area"]), pi["avg_depth"]
    return o


def compare_with_fields(got, o, what=""):
    """the restatement's (or the GPU's) dict against scalar_fields' arrays (or a golden set): every field the scalar functions return,
    bit for bit"""
    keep, reason = o["keep"].astype(bool), o["reason"].astype(np.int64)
    assert np.array_equal(got["keep"].astype(bool), keep), what
    assert np.array_equal(got["reason"], reason), what
    valid, miss, small = reason == 0, reason == 3, reason == 4
    assert np.array_equal(got["corners_in_view"][valid | miss], o["corners_in_view"][valid | miss]), what
    assert np.array_equal(got["corners_near"][valid], o["corners_near"][valid]), what
    assert same_bits(got["avg_depth"][valid], o["avg_depth"][valid]), what
    nb = got["near_bbox2d"]
    assert np.array_equal(nb[miss], o["bbox_2d"][miss].astype(np.float64)), what
    ur, vr = nb[small, 2] - nb[small, 0], nb[small, 3] - nb[small, 1]
    assert np.array_equal(np.stack([ur * vr, ur, vr], axis=1), o["small"][small].astype(np.float64)), what
    assert (got["corners_near"][reason == 2] == 0).all(), what
    ok = o["proj_ok"].astype(bool)
    assert np.array_equal(got["front"] > 0, ok), what
    bb = got["bbox2d"][ok]
    assert np.array_equal(bb, o["proj_bbox"][ok].astype(np.float64)), what
    assert np.array_equal(np.stack([(bb[:, 0] + bb[:, 2]) / 2, (bb[:, 1] + bb[:, 3]) / 2], axis=1), o["proj_center"][ok]), what
    assert np.array_equal(np.stack([bb[:, 2] - bb[:, 0], bb[:, 3] - bb[:, 1]], axis=1), o["proj_size"][ok].astype(np.float64)), what
    assert np.array_equal((bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1]), o["proj_area"][ok].astype(np.float64)), what
    assert same_bits(got["front_avg_depth"][ok], o["proj_avg_depth"][ok]), what
    assert (got["bbox2d"][~ok] == [BIG, BIG, -BIG, -BIG]).all() and (got["front_avg_depth"][~ok] == 0).all(), what


def seeded_boxes(n, seed=0):
    """the seeded boxes of golden set (b): float64 [n,8,3] cam-0 corners"""
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(-60, 60, n), rng.uniform(-2, 3, n), rng.uniform(-20, 140, n)], axis=1)
    extent = np.array([1.65, 1.97, 4.43]) * rng.uniform(0.05, 1.2, n)[:, None]
    sign = rng.integers(0, 2, (n, 8, 3)) * 2.0 - 1.0
    return centre[:, None, :] + sign * (extent[:, None, :] / 2)
