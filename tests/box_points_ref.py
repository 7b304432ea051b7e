"""Per-box LiDAR point counts and point-level recall, restated in NumPy from oracle/numpy_path (TEST ONLY): what lpf_box_points,
LpfContext.box_points and pipeline.point_recall_frames are compared with.  The membership test is the reference's own expression on
points_valid = points[valid_indices, :3] (V3:590-592): oracle.numpy_path.oriented_point_in_bbox (V3:167-204) or point_in_bbox
(V3:143-164, as tests/inside_ref.py restates it); the first box of a point is the lowest index whose boolean array holds it.
tests/test_box_points_api.py pins the sums and the first boxes against arrays the reference itself produced
(tests/golden/box_points_golden.npz)."""
import numpy as np

import inside_ref as IR
from oracle import numpy_path as NP

WINDOWS = (("d50", 50.0), ("d30", 30.0))
KINDS = (("oriented", True), ("aabb", False))


def valid_indices(points, T, K3, W, H, dmax):
    """V3:565-569 + V3:584-585: the indices of the points that project into the image with 0 < depth < dmax"""
    points_homo = points.copy()
    points_homo[:, 3] = 1
    pointsCam = np.matmul(T, points_homo.T).T[:, :3]
    u, v, depth = NP.cam2image(K3, pointsCam.T)
    return np.where((u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth > 0) & (depth < dmax))[0].astype(np.int64)


def membership(points_valid, corners, oriented=True):
    """bool [B, k]: row b is the reference's boolean array of box b over points_valid"""
    k = len(points_valid)
    out = np.zeros((len(corners), k), bool)
    if k:
        for b, c in enumerate(corners):
            out[b] = IR.inside_one(points_valid, c, oriented)
    return out


def first_box_of(inside):
    """int32 [k]: the lowest b with inside[b, i], -1 if no box holds point i"""
    if inside.shape[0] == 0:
        return np.full(inside.shape[1], -1, np.int32)
    return np.where(inside.any(axis=0), inside.argmax(axis=0), -1).astype(np.int32)


def frame_box_points(points, valid_idx, corners, labelled=None, oriented=True, enabled=None):
    """One frame: ``points`` float32 [N,4], ``valid_idx`` int64 [k] ascending, ``corners`` f64 [B,8,3], ``labelled`` bool [k] (None:
    nothing is labelled), ``enabled`` bool [B] (None: every box; a box that is not enabled holds nothing).  Returns box_points int32
    [B], box_labelled int32 [B], first_box int32 [k], frame_counts int64 [4] = {valid, in >= 1 box, labelled, labelled and in >= 1
    box} and ``inside`` bool [B, k]."""
    valid_idx = np.asarray(valid_idx, np.int64)
    lab = np.zeros(len(valid_idx), bool) if labelled is None else np.asarray(labelled, bool)
    inside = membership(points[valid_idx, :3], corners, oriented)
    if enabled is not None:
        inside &= np.asarray(enabled, bool)[:, None]
    anyb = inside.any(axis=0) if len(corners) else np.zeros(len(valid_idx), bool)
    return dict(box_points=inside.sum(axis=1).astype(np.int32), box_labelled=(inside & lab[None, :]).sum(axis=1).astype(np.int32),
                first_box=first_box_of(inside), inside=inside,
                frame_counts=np.array([len(valid_idx), anyb.sum(), lab.sum(), (anyb & lab).sum()], np.int64))


def batch_box_points(frames, valid, corners, labelled=None, oriented=True):
    """The four arrays of a batch as lpf_box_points lays them out: box_points / box_labelled int32 [Btot], first_box int32 [Ntot]
    (frame f's from frame_off[f], -1 where the call writes nothing) and frame_counts int64 [F,4]."""
    off = np.concatenate([[0], np.cumsum([len(p) for p in frames])]).astype(np.int64)
    first = np.full(int(off[-1]), -1, np.int32)
    bp, bl, fc = [], [], np.zeros((len(frames), 4), np.int64)
    for f, (p, vi, c) in enumerate(zip(frames, valid, corners)):
        r = frame_box_points(p, vi, c, None if labelled is None else labelled[f], oriented)
        bp.append(r["box_points"]); bl.append(r["box_labelled"]); fc[f] = r["frame_counts"]
        first[off[f]:off[f] + len(vi)] = r["first_box"]
    cat = lambda x: np.concatenate(x).astype(np.int32) if x else np.zeros(0, np.int32)
    return dict(box_points=cat(bp), box_labelled=cat(bl), first_box=first, frame_counts=fc)


def confusion(frame_counts):
    """{"tp", "fp", "fn", "tn"} of "car vs. not car" per point: labelled = predicted, in a box = ground truth"""
    valid, boxed, lab, both = (int(x) for x in frame_counts)
    return {"tp": both, "fp": lab - both, "fn": boxed - both, "tn": valid - boxed - lab + both}


def labelled_of(valid_idx, lists):
    """bool [k]: the valid points some instance list holds (V4:290-298's bg_assigned)"""
    lab = np.zeros(len(valid_idx), bool)
    for l in lists:
        lab |= np.isin(valid_idx, l)
    return lab


def recall_frame(points, valid_idx, lists, corners, colors, min_points=10, oriented=True):
    """What pipeline.point_recall_frames adds to run_frames' dict of one frame whose box list is ``corners`` (positions 0 .. B-1):
    box_points, box_labelled, first_box, point_confusion, and car_statistics (cvs_erosion's key set) with bbox_lidar_points and
    recall_percentage."""
    r = frame_box_points(points, valid_idx, corners, labelled_of(valid_idx, lists), oriented)
    stats = []
    if len(corners) and len(lists):
        sp = IR.frame_split(points, lists, corners, min_points, oriented)
        for m, l in enumerate(lists):
            total = len(l)
            if total == 0:
                continue
            if sp["matched"][m]:
                ins, bb = int(sp["best_cnt"][m]), int(sp["best_box"][m])
                n_box = int(r["box_points"][bb])
                stats.append({"car_id": m, "matched_bbox_id": bb, "total_points": total, "points_inside_bbox": ins,
                              "points_outside_bbox": total - ins, "inside_percentage": (ins / total) * 100,
                              "outside_percentage": ((total - ins) / total) * 100, "color": colors[m],
                              "bbox_lidar_points": n_box, "recall_percentage": ins / n_box * 100})
            else:
                stats.append({"car_id": m, "matched_bbox_id": -1, "total_points": total, "points_inside_bbox": 0,
                              "points_outside_bbox": total, "inside_percentage": 0.0, "outside_percentage": 100.0, "color": colors[m],
                              "bbox_lidar_points": 0, "recall_percentage": 0.0})
    return dict(box_points=r["box_points"], box_labelled=r["box_labelled"], first_box=r["first_box"],
                point_confusion=confusion(r["frame_counts"]), car_statistics=stats, frame_counts=r["frame_counts"])


def golden_case(g, window):
    """(points, valid_idx, corners) of a committed sub-sampled golden frame (tests/golden/frame_*.npz) under depth window ``window``;
    a frame without a box file has neither boxes nor stored indices: its valid indices are restated from the calibration by the caller"""
    corners = g["corners_velo"] if "corners_velo" in g else np.zeros((0, 8, 3))
    return g["points"], g.get("valid_idx_" + window), corners
