"""V3's inside / outside split, restated in NumPy from oracle/numpy_path (TEST ONLY): what lpf_inside_masks, car_statistics_v3_frames and
inside_outside_cloud_frames are compared with.  The membership test is the reference's own expression (oracle.numpy_path.
oriented_point_in_bbox, V3:167-204; point_in_bbox, V3:143-164, restated here the same way); the best box is the first strict maximum of
the counts (V3:353-376); the parts are the boolean gathers of V3:494 and V3:502.  tests/test_inside_api.py pins all of it against
masks the reference itself produced (tests/golden/inside_golden.npz)."""
import numpy as np

from oracle import numpy_path as NP


def point_in_bbox(points, c):
    """V3:143-164: inside the axis-aligned hull of the 8 corners, closed"""
    if len(points) == 0:
        return np.array([])
    return np.all((points >= np.min(c, axis=0)) & (points <= np.max(c, axis=0)), axis=1)


def inside_one(points, c, oriented=True):
    return NP.oriented_point_in_bbox(points, c) if oriented else point_in_bbox(points, c)


def car_sets(points, lists):
    """V3:228: one float32 [k,3] array per list of point indices"""
    return [points[np.asarray(l, np.int64), :3] if len(l) else np.array([]).reshape(0, 3) for l in lists]


def frame_split(points, lists, corners, min_points=10, oriented=True):
    """One frame: ``points`` float32 [N,4], ``lists`` the M instance lists (point indices, ascending), ``corners`` f64 [B,8,3].
    Returns count_mb int64 [M,B], best_box int32 [M], best_cnt int64 [M], off int64 [M+1] and, over the concatenated lists,
    inside uint8, part_idx int64, part_xyz float32 [.,3], plus n_inside int64 [M] and matched int32 [M]."""
    M, B = len(lists), len(corners)
    sets = car_sets(points, lists)
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    count = np.zeros((M, B), np.int64)
    best_box, best_cnt = np.full(M, -1, np.int32), np.zeros(M, np.int64)
    inside = np.zeros(int(off[-1]), np.uint8)
    part_idx = np.zeros(int(off[-1]), np.int64)
    part_xyz = np.zeros((int(off[-1]), 3), np.float32)
    n_inside, matched = np.zeros(M, np.int64), np.zeros(M, np.int32)
    for m, (l, s) in enumerate(zip(lists, sets)):
        l = np.asarray(l, np.int64)
        best_mask = None
        if len(s):
            for b in range(B):
                msk = inside_one(s, corners[b], oriented)
                count[m, b] = int(np.sum(msk))
                if count[m, b] > best_cnt[m]:
                    best_cnt[m], best_box[m], best_mask = count[m, b], b, msk
        a, e = int(off[m]), int(off[m + 1])
        if best_box[m] >= 0 and best_cnt[m] >= min_points:
            matched[m], n_inside[m] = 1, best_cnt[m]
            inside[a:e] = best_mask
            part_idx[a:e] = np.concatenate([l[best_mask], l[~best_mask]])
            part_xyz[a:e] = np.concatenate([s[best_mask], s[~best_mask]])
        elif len(s):
            part_idx[a:e], part_xyz[a:e] = l, s
    return dict(count_mb=count, best_box=best_box, best_cnt=best_cnt, off=off, inside=inside, part_idx=part_idx, part_xyz=part_xyz,
                n_inside=n_inside, matched=matched)


def v3_statistics(points, lists, bboxes_3d, colors, min_points=10, oriented=True):
    """V3:320-428 without its prints: the statistics dicts with V3's key set.  bboxes_3d: dicts with 'corners_velo'."""
    stats = []
    if not bboxes_3d or len(lists) == 0:
        return stats
    corners = np.array([b["corners_velo"] for b in bboxes_3d], np.float64).reshape(-1, 8, 3)
    sp = frame_split(points, lists, corners, min_points, oriented)
    for m, s in enumerate(car_sets(points, lists)):
        total = len(s)
        if total == 0:
            continue
        a, e = int(sp["off"][m]), int(sp["off"][m + 1])
        if sp["matched"][m]:
            ins = int(sp["best_cnt"][m])
            stats.append({"car_id": m, "matched_bbox_id": int(sp["best_box"][m]), "total_points": total, "points_inside_bbox": ins,
                          "points_outside_bbox": total - ins, "inside_percentage": (ins / total) * 100,
                          "outside_percentage": ((total - ins) / total) * 100, "color": colors[m],
                          "corners_velo": np.array(bboxes_3d[int(sp["best_box"][m])]["corners_velo"]),
                          "inside_mask": sp["inside"][a:e] != 0, "car_points": s})
        else:
            stats.append({"car_id": m, "matched_bbox_id": -1, "total_points": total, "points_inside_bbox": 0, "points_outside_bbox": total,
                          "inside_percentage": 0.0, "outside_percentage": 100.0, "color": colors[m], "corners_velo": None,
                          "inside_mask": None, "car_points": s})
    return stats


def cloud(stats, points_valid, bg_assigned, background=(0.5, 0.5, 0.5)):
    """V3:471-515 + V3:618-621 as arrays: points float32 [n,3], colors float64 [n,3], parts int32 [n,2] = (car id, 0 unmatched /
    1 inside / 2 outside / 3 background with car id -1), geometry after geometry in the reference's order."""
    pts, cols, parts = [], [], []

    def add(p, color, car, code):
        pts.append(np.asarray(p, np.float32).reshape(-1, 3))
        cols.append(np.tile(np.asarray(color, np.float64), (len(p), 1)).reshape(-1, 3))
        parts.append(np.tile(np.array([[car, code]], np.int32), (len(p), 1)))
    for s in stats:
        color = np.array([s["color"][2], s["color"][1], s["color"][0]]) / 255.0
        if s["matched_bbox_id"] < 0:
            add(s["car_points"], color, s["car_id"], 0)
            continue
        m = s["inside_mask"]
        if np.any(m):
            add(s["car_points"][m], color, s["car_id"], 1)
        if np.any(~m):
            add(s["car_points"][~m], color, s["car_id"], 2)
    rest = np.asarray(points_valid)[~np.asarray(bg_assigned, bool)]
    add(rest, background, -1, 3)
    return dict(points=np.concatenate(pts), colors=np.concatenate(cols), parts=np.concatenate(parts))


def golden_frame_case(g, tag, calib=None):
    """(points, lists, corners) of a committed golden frame (tests/golden/frame_*.npz) under ``tag``"""
    counts = g["inst_count_" + tag] if ("inst_count_" + tag) in g else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cat = g["inst_cat_" + tag] if len(counts) else np.zeros(0, np.int64)
    lists = [cat[a:b] for a, b in zip(off[:-1], off[1:])]
    corners = g["corners_velo"] if "corners_velo" in g else np.zeros((0, 8, 3))
    return g["points"], lists, corners
