"""The reference's function surface for the hot path, served by the HIP library.

Names, argument meaning, return types and print formats follow
``Coding_testes/V3_point_cloud_with_erosion.py`` / ``cvs_erosion.py`` /
``V4_BBox_IoU_filtering.py`` (paths relative to /root/reference; line numbers cited per
function).  Everything that touches per-point data goes through ``liblpf.so``
(``_native.LpfContext``); what stays on the host is box-level scalar logic (8 corners per
box), dict assembly, printing and CSV -- none of it is a fallback for the kernels, and
there is no CPU path for them: without the GPU library these functions raise.

YOLO segmentation and Open3D stay outside (reference: unchanged subsystems); the entry
points take them as callables.
"""
import contextlib
import io
import os
import sys
from datetime import datetime

import numpy as np

from . import _native, kitti360
from ._native import LpfContext, LPF_MAX_CAMS, LPF_MAX_MASKS, LPF_MAX_MASKS_WIDE, Scan, ScanReader
from .idmap import IdMasks
from .rle import RleMasks

_CONTEXTS = {}


def get_context(device=0):
    """Process-wide LpfContext of one GPU (created on first use)."""
    ctx = _CONTEXTS.get(device)
    if ctx is None:
        ctx = _CONTEXTS[device] = LpfContext(device)
    return ctx


def _erosion_kernel_size(k):
    """``erosion_kernel_size`` (V3:55, cvs_erosion.py:77: the side of the MORPH_ELLIPSE element) as the library takes it: an odd
    integer 1 .. 15 (lpf_set_erosion_element), anything else raises ValueError -- before any GPU work."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 15 or k % 2 == 0:
        raise ValueError("erosion_kernel_size must be an odd integer from 1 to 15 (the k x k MORPH_ELLIPSE element), got %r" % (k,))
    return int(k)


def _f32_points(points, what="points"):
    """float32 view of caller points; refuses values a float32 cannot hold (the kernels
    take the velodyne float32 format, V3:28, and there is no float64 point path)."""
    p = np.asarray(points)
    if p.dtype == np.float32:
        return np.ascontiguousarray(p)
    q = np.ascontiguousarray(p, dtype=np.float32)
    if not np.array_equal(q.astype(np.float64), np.asarray(p, dtype=np.float64), equal_nan=True):
        raise TypeError("%s must hold float32-representable values (velodyne .bin format)" % what)
    return q


def _is_device_tensor(x):
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _mask_stack(masks, camera, resize_ctx=None, erode_iters=0, v3_pipeline=False, force_chain=False, erosion_kernel_size=3):
    """([M,H,W] float32/uint8 array from the reference's mask list, eroded_already).  A torch tensor that is already on the GPU --
    ``result.masks.data`` before the reference's ``.cpu().numpy()`` (V3:72) -- is passed through: the kernels read it where it is.
    Masks that do not arrive at the camera's size (the reference's scripts pass retina_masks=True, V3:64, so theirs do) go through
    ``cv2.resize(mask.astype(np.uint8), (W, H))`` as V3:222 does it -- on the GPU, by ``resize_ctx`` (whose camera must have been
    set; LpfContext.resize_masks) -- and come back as uint8 [M,H,W], nonzero = the reference's ``> 0.5``.  With the V3 erosion block
    in force (``v3_pipeline`` / ``erode_iters``) such masks take V3's own order: ``(mask * 255).astype(uint8)`` -> ``cv2.erode`` AT THE
    MASKS' OWN SIZE -> ``/ 255.0`` (V3:82-97), and only then ``astype(uint8)`` + resize (V3:222) -- all on the GPU
    (LpfContext.erode_masks, then resize_masks); the second value tells the caller that the erosion has been done.  ``force_chain``:
    masks at camera size take the same explicit chain (a batch is eroded either all inside lpf_set_masks_* or all here).
    ``erosion_kernel_size``: the side of the erosion's MORPH_ELLIPSE element (V3:55), set on ``resize_ctx`` before it erodes."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)

    def chain(m):
        """off-size masks -> uint8 [M,H,W] at camera size (device tensor in -> device tensor out)"""
        if resize_ctx is None:
            raise NotImplementedError("masks must already be %dx%d (retina_masks=True, V3:64) in this call" % (camera.height, camera.width))
        if not (erode_iters or v3_pipeline):
            return resize_ctx.resize_masks(m), False
        resize_ctx.set_erosion_element(erosion_kernel_size)
        dev = _is_device_tensor(m)
        if dev:
            import torch
            f = m.to(torch.float32)
            u8 = (f * 255).to(torch.uint8) if v3_pipeline else f.to(torch.uint8)       # (mask * 255).astype(np.uint8), V3:85
            er = resize_ctx.erode_masks(u8.contiguous(), erode_iters)                 # cv2.erode at the masks' own size, V3:86-90
            back = (er == 255).to(torch.uint8) if v3_pipeline else er                 # / 255.0 (V3:93) then astype(np.uint8) (V3:222): 1 only for 255
        else:
            f = np.asarray(m)
            u8 = (f.astype(np.float32) * 255).astype(np.uint8) if v3_pipeline else f.astype(np.uint8)
            er = resize_ctx.erode_masks(u8, erode_iters)
            back = (er.astype(np.float32) / 255.0).astype(np.uint8) if v3_pipeline else er
        return resize_ctx.resize_masks(back), True
    if _is_device_tensor(masks):
        import torch
        if masks.ndim != 3:
            raise ValueError("device masks must be [M,h,w]")
        if tuple(masks.shape[1:]) != (camera.height, camera.width) or (force_chain and masks.shape[0]):
            return chain(masks)
        if masks.dtype == torch.bool:
            masks = masks.to(torch.uint8)
        elif masks.dtype not in (torch.float32, torch.uint8):
            masks = masks.to(torch.float32)
        return masks.contiguous(), False
    m = np.asarray(masks)
    if m.size == 0:
        return np.zeros((0, camera.height, camera.width), np.uint8), False
    if m.ndim != 3:
        raise ValueError("masks must be [M,h,w]")
    if m.shape[1:] != (camera.height, camera.width) or force_chain:
        return chain(m)
    if m.dtype.kind == "f":
        return np.ascontiguousarray(m, dtype=np.float32), False
    return np.ascontiguousarray(m.astype(np.uint8)), False


# ---------------------------------------------------------------------------------------
# box preparation (host scalars: 8 corners per box)
# ---------------------------------------------------------------------------------------
def filter_visible_bboxes(bboxes_3d, camera):
    """Keep boxes with >= 2 corners in front (depth > 0.1) and inside the image (V3:121-140).
    As in the reference the corners are projected without R_rect."""
    filtered = []
    for bbox in bboxes_3d:
        if "corners_cam0" not in bbox:
            continue
        corners = np.array(bbox["corners_cam0"])
        u, v, depth = camera.cam2image(corners.T)
        ok = (depth > 0.1) & (u >= 0) & (u < camera.width) & (v >= 0) & (v < camera.height)
        if np.sum(ok) >= 2:
            filtered.append(bbox)
    return filtered


def transform_bboxes_to_velodyne(bboxes_3d, TrVeloToCam):
    """Adds 'corners_velo' (list) to every box dict, in place (V3:41-52)."""
    cam_to_velo = np.linalg.inv(TrVeloToCam)
    for bbox in bboxes_3d:
        if "corners_cam0" in bbox:
            c = np.array(bbox["corners_cam0"])
            homo = np.hstack([c, np.ones((c.shape[0], 1))])
            bbox["corners_velo"] = np.matmul(cam_to_velo, homo.T).T[:, :3].tolist()
    return bboxes_3d


def prepare_boxes(bboxes_3d_raw, camera, TrVeloToCam, device=0, keep_all=False, as_arrays=False):
    """filter_visible_bboxes + transform_bboxes_to_velodyne (+ V4's projected 2D box) in one GPU call
    (SURVEY 8f-1): returns the visible boxes, in order, each a copy of the input dict with
    'corners_velo' (list, as the reference stores it) and '_bbox2d' / '_front' for the IoU match.
    The camera of the context is set to (camera.K, width, height).  ``keep_all=True`` skips the
    visibility filter (V5 transforms every box, V5:454-461).  ``as_arrays=True`` (callers that keep the boxes to themselves, like
    process_frames, whose only product is the CSV) stores 'corners_velo' as the f64 [8,3] array instead of the reference's
    ``.tolist()`` of it -- the same values; 7 500 Python floats per frame of 314 boxes that nobody reads cost more than the frame's kernels."""
    have = [b for b in bboxes_3d_raw if "corners_cam0" in b]
    if not have:
        return []
    ctx = get_context(device)
    ctx.ensure_intrinsics(camera.K, camera.width, camera.height)
    corners = np.array([b["corners_cam0"] for b in have], np.float64).reshape(-1, 8, 3)
    vis, cv, bb, fr = ctx.prepare_boxes(corners, np.linalg.inv(TrVeloToCam))
    out = _PreparedBoxes()
    bb_l, fr_l, vis_l = bb.tolist(), fr.tolist(), vis.tolist()      # (one conversion each: per box it cost more than the kernels)
    cv_l = cv if as_arrays else cv.tolist()
    for i, b in enumerate(have):
        if vis_l[i] or keep_all:
            d = dict(b)
            d["corners_velo"] = cv_l[i]
            d["_cv"] = cv[i]                                 # the same values as an array (private: spares run_frames the way back from lists)
            d["_bbox2d"] = bb_l[i] if fr_l[i] > 0 else None
            d["_front"] = fr_l[i]
            out.append(d)
    out.cv = cv if keep_all else cv[vis]
    return out


class _PreparedBoxes(list):
    """prepare_boxes' list of box dicts, with the corners of all of them as ONE float64 [B,8,3] array beside it (``cv``: what
    run_frames hands to the GPU, without a walk over the dicts).  A list in every other respect; ``cv`` is dropped by anything that
    makes a new list of it (slices, filters), and ``_corners_velo`` only trusts it while the lengths agree."""
    __slots__ = ("cv",)

    def __init__(self, *a):
        super().__init__(*a)
        self.cv = None


def prepare_boxes_from_arrays(index, corners_cam0, camera, TrVeloToCam, device=0, keep_all=False):
    """prepare_boxes for a box file the library has parsed (lpf_parse_boxes_json / the read-ahead reader: ``index`` int32 [B],
    ``corners_cam0`` float64 [B,8,3] -- the doubles json.load gives): the visible boxes, in order, as dicts with 'index',
    'corners_velo' (the f64 [8,3] array, as prepare_boxes(as_arrays=True) stores it), '_bbox2d' / '_front'.  The cam-0 corners are
    not copied into per-box lists: this is the form for callers that keep the boxes to themselves (process_frames)."""
    corners = np.ascontiguousarray(corners_cam0, dtype=np.float64).reshape(-1, 8, 3)
    out = _PreparedBoxes()
    if not len(corners):
        return out
    ctx = get_context(device)
    ctx.ensure_intrinsics(camera.K, camera.width, camera.height)
    vis, cv, bb, fr = ctx.prepare_boxes(corners, np.linalg.inv(TrVeloToCam))
    keep = np.arange(len(corners)) if keep_all else np.flatnonzero(vis)
    idx_l, bb_l, fr_l = np.asarray(index)[keep].tolist(), bb[keep].tolist(), fr[keep].tolist()
    out.cv = cv[keep]
    for j in range(len(keep)):
        c = out.cv[j]
        out.append({"index": idx_l[j], "corners_velo": c, "_cv": c, "_bbox2d": bb_l[j] if fr_l[j] > 0 else None, "_front": fr_l[j]})
    return out


def _corners_velo(bboxes_3d):
    """f64 [B,8,3] of the boxes that carry 'corners_velo' + their positions in the list."""
    if isinstance(bboxes_3d, _PreparedBoxes) and bboxes_3d.cv is not None and len(bboxes_3d.cv) == len(bboxes_3d):
        return bboxes_3d.cv, list(range(len(bboxes_3d)))     # (every dict of prepare_boxes carries 'corners_velo')
    pos = [i for i, b in enumerate(bboxes_3d) if "corners_velo" in b]
    if not pos:
        return np.zeros((0, 8, 3)), pos
    if all("_cv" in bboxes_3d[i] for i in pos):             # boxes that come from prepare_boxes carry their corners as arrays too
        return np.stack([bboxes_3d[i]["_cv"] for i in pos]).reshape(-1, 8, 3), pos
    return np.array([bboxes_3d[i]["corners_velo"] for i in pos], np.float64).reshape(-1, 8, 3), pos


# ---------------------------------------------------------------------------------------
# projection + clip (reference: inline statements V3:565-569 and V3:584-592)
# ---------------------------------------------------------------------------------------
def project_points(points, TrVeloToRect, camera, depth_max=50.0, want_depth=True, device=0):
    """(u, v, depth, valid_indices) of f32[N,4] velodyne points: u, v int64 as in the reference
    (``np.round(...).astype(int)``), depth float64 (None unless want_depth), valid_indices =
    ``np.where(valid)[0]``."""
    ctx = get_context(device)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    ctx.clear_masks()
    ctx.clear_boxes()
    r = ctx.run(_f32_points(points).reshape(-1, 4), want_float=want_depth, want_label=False)
    return r["u"].astype(np.int64), r["v"].astype(np.int64), (r["depth"] if want_depth else None), r["valid_idx"]


def per_car_depth_maps(points, TrVeloToRect, camera, masks, depth_max=30.0, device=0):
    """[(car_id, depthMap f64[H,W])] as seg_with_pointcloud.py:160-170 builds them (car_id = i + 1,
    ``depthMap[v,u] = depth`` of the last valid point in mask i at that pixel, 0 elsewhere).  The
    scatter -- a Python loop over every valid point per mask in the reference -- runs once on the
    GPU (the winner of a pixel does not depend on the mask); the per-mask select is elementwise."""
    ctx = get_context(device)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    D, _ = ctx.depth_image(_f32_points(points).reshape(-1, 4))
    return [(i + 1, np.where(np.asarray(m) > 0.5, D, 0.0)) for i, m in enumerate(masks)]


class SparseDepthMap:
    """One car's depth map of seg_with_pointcloud.py:160-170 as the list of its nonzero pixels: ``pixels`` = the flat indices
    v * W + u in ascending order (``np.flatnonzero(depthMap)``), ``depth`` = ``depthMap.ravel()[pixels]``, ``point_idx`` = the
    winning point of each pixel (index into the frame's scan, or None), ``shape`` = (H, W).  to_dense() is the script's depthMap."""
    __slots__ = ("car_id", "pixels", "depth", "point_idx", "shape")

    def __init__(self, car_id, pixels, depth, point_idx, shape):
        self.car_id, self.pixels, self.depth, self.point_idx, self.shape = car_id, pixels, depth, point_idx, tuple(shape)

    def to_dense(self):
        """depthMap f64 [H,W]: depth at the listed pixels, 0 elsewhere"""
        d = np.zeros(self.shape, np.float64)
        d.ravel()[self.pixels] = self.depth
        return d

    def __len__(self):
        return len(self.pixels)

    def __repr__(self):
        return "SparseDepthMap(car_id=%d, %d pixels, shape=%s)" % (self.car_id, len(self.pixels), self.shape)


# ---------------------------------------------------------------------------------------
# mask lookup (V3:211-233, cvs_erosion.py:148-162)
# ---------------------------------------------------------------------------------------
def extract_car_points_by_mask(points_valid, u_valid, v_valid, masks, camera, device=0):
    """One point array per mask: ``points_valid[mask[v_valid, u_valid] > 0.5]``, empty masks give
    a (0,3) float64 array.  The pixels are looked up by the same kernel the fused path uses
    (run on the already-projected pixels with an identity camera)."""
    pv = np.asarray(points_valid)
    n = pv.shape[0]
    ctx = get_context(device)
    ctx.set_camera(np.eye(4), np.eye(3), camera.width, camera.height, 0.0, 2.0)
    stack, _ = _mask_stack(masks, camera, resize_ctx=ctx)    # (V3:222: masks of another size are resized, on the GPU)
    M = stack.shape[0]
    sets = []
    if M == 0:
        return sets
    pix = np.zeros((n, 4), np.float32)
    pix[:, 0] = np.asarray(u_valid)
    pix[:, 1] = np.asarray(v_valid)
    pix[:, 2] = 1.0
    ctx.clear_boxes()
    if M <= LPF_MAX_MASKS:
        ctx.set_masks(stack)
        r = ctx.run(pix, want_uv=False, want_label=False)
        lists = r["inst_lists"]
    else:                                                    # more detections: the wide pass (groups of 256 beyond that)
        lists = []
        for m0 in range(0, M, LPF_MAX_MASKS_WIDE):
            lists += ctx.run_wide([pix], stack[m0:m0 + LPF_MAX_MASKS_WIDE], want_uv=False)[0]["inst_lists"]
    for lst in lists:
        sets.append(pv[lst] if len(lst) else np.array([]).reshape(0, 3))
    return sets


# ---------------------------------------------------------------------------------------
# box membership (V3:143-208)
# ---------------------------------------------------------------------------------------
def oriented_point_in_bbox(points, bbox_corners, device=0):
    """bool[k]: inside the three slabs c1-c0, c3-c0, c4-c0 (closed), as V3:167-204."""
    if len(points) == 0:
        return np.array([])
    p = _f32_points(points)
    return get_context(device).points_in_boxes(p, np.asarray(bbox_corners, np.float64)[None], oriented=True)[0]


def point_in_bbox(points, bbox_corners, device=0):
    """bool[k]: inside the axis-aligned hull of the 8 corners (closed), as V3:143-164."""
    if len(points) == 0:
        return np.array([])
    p = _f32_points(points)
    return get_context(device).points_in_boxes(p, np.asarray(bbox_corners, np.float64)[None], oriented=False)[0]


def _count_matrix(car_point_sets, corners, use_oriented, device=0, want_masks=False):
    """counts[car, box] (+ the per-point inside matrix and set offsets) with ONE kernel call."""
    sizes = [len(s) for s in car_point_sets]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    B = corners.shape[0]
    counts = np.zeros((len(sizes), B), np.int64)
    inside = None
    if off[-1] and B:
        cat = np.concatenate([_f32_points(s).reshape(-1, 3) for s in car_point_sets if len(s)], axis=0)
        inside = get_context(device).points_in_boxes(cat, corners, oriented=use_oriented)
        csum = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(inside, axis=1, dtype=np.int64)], axis=1)
        counts = (csum[:, off[1:]] - csum[:, off[:-1]]).T.copy()
    return counts, (inside if want_masks else None), off


def _best_box(counts_row):
    """First strict maximum starting from 0 (V3:353-376): (-1, 0) when no box holds a point."""
    best, idx = 0, -1
    for b, c in enumerate(counts_row):
        if c > best:
            best, idx = int(c), b
    return idx, best


def match_car_points_to_bboxes(car_point_sets, bboxes_3d, colors, min_points=10, use_oriented=True, device=0):
    """[(corners_velo, rgb_color, count)] for the matched cars (V3:236-290)."""
    matched = []
    if not bboxes_3d or len(car_point_sets) == 0:
        return matched
    corners, pos = _corners_velo(bboxes_3d)
    counts, _, _ = _count_matrix(car_point_sets, corners, use_oriented, device)
    for car_idx, car_points in enumerate(car_point_sets):
        if len(car_points) == 0:
            continue
        best, best_idx = 0, -1
        for j, c in enumerate(counts[car_idx]):
            if c > best and c >= min_points:
                best, best_idx = int(c), pos[j]
        if best_idx >= 0:
            col = colors[car_idx]
            matched.append((np.array(bboxes_3d[best_idx]["corners_velo"]), np.array([col[2], col[1], col[0]]) / 255.0, best))
            print(f"  Matched car {car_idx} to bbox {best_idx} with {best} points")
    return matched


def stats_from_counts(car_sizes, counts, colors, min_points=10, box_positions=None):
    """The reference's per-car dicts (cvs_erosion.py:165-229 key set) from integer counts:
    car_sizes[m] = len(car_point_sets[m]), counts[m, b] = points of car m inside box b."""
    out = []
    for car_idx, total in enumerate(car_sizes):
        total = int(total)
        if total == 0:
            continue
        j, best = _best_box(counts[car_idx]) if counts.shape[1] else (-1, 0)
        if j >= 0 and best >= min_points:
            inside, outside = best, total - best
            out.append({"car_id": car_idx, "matched_bbox_id": box_positions[j] if box_positions is not None else j,
                        "total_points": total, "points_inside_bbox": inside, "points_outside_bbox": outside,
                        "inside_percentage": (inside / total) * 100, "outside_percentage": (outside / total) * 100,
                        "color": colors[car_idx], "_best_col": j, "_best_count": best})
        else:
            out.append({"car_id": car_idx, "matched_bbox_id": -1, "total_points": total, "points_inside_bbox": 0,
                        "points_outside_bbox": total, "inside_percentage": 0.0, "outside_percentage": 100.0,
                        "color": colors[car_idx], "_best_col": -1, "_best_count": best})
    return out


def calculate_car_point_statistics(car_point_sets, bboxes_3d, colors, min_points=10, use_oriented=True,
                                   style="v3", device=0):
    """Per-car inside/outside statistics (V3:320-428; ``style='cvs'`` gives cvs_erosion.py:165-229's
    quieter variant without the array-valued keys).  Cars with no points get no row."""
    stats = []
    if not bboxes_3d or len(car_point_sets) == 0:
        return stats
    v3 = style == "v3"
    if v3:
        print(f"\n=== Car Point Statistics ===")
    print(f"Total car detections: {len(car_point_sets)}")
    print(f"Total 3D bounding boxes: {len(bboxes_3d)}")
    corners, pos = _corners_velo(bboxes_3d)
    counts, inside, off = _count_matrix(car_point_sets, corners, use_oriented, device, want_masks=v3)
    rows = stats_from_counts([len(s) for s in car_point_sets], counts, colors, min_points, pos)
    by_car = {r["car_id"]: r for r in rows}
    for car_idx, car_points in enumerate(car_point_sets):
        total = len(car_points)
        if total == 0:
            if v3:
                print(f"\nCar {car_idx}: No points detected")
            continue
        r = by_car[car_idx]
        j, best = r.pop("_best_col"), r.pop("_best_count")
        if v3:
            print(f"\nCar {car_idx}: {total} total points")
            if r["matched_bbox_id"] >= 0:
                r["corners_velo"] = np.array(bboxes_3d[r["matched_bbox_id"]]["corners_velo"])
                r["inside_mask"] = inside[j, off[car_idx]:off[car_idx + 1]]
                print(f"  ✓ Matched to 3D bbox {r['matched_bbox_id']}")
                print(f"  │ Points inside bbox:  {r['points_inside_bbox']:4d} ({r['inside_percentage']:5.1f}%)")
                print(f"  │ Points outside bbox: {r['points_outside_bbox']:4d} ({r['outside_percentage']:5.1f}%)")
                print(f"  └ Total points:        {total:4d} (100.0%)")
            else:
                r["corners_velo"] = None
                r["inside_mask"] = None
                print(f"  ✗ No matching 3D bbox found (best match: {best} points < {min_points} threshold)")
            r["car_points"] = car_points
        stats.append(r)
    return stats


# ---------------------------------------------------------------------------------------
# 2D IoU matching of V4 (V4:118-183) and V5 (V5:277-416), one frame at a time in host scalars: the yardstick of the batched forms below
# ---------------------------------------------------------------------------------------
def calculate_iou_2d(box1, box2):
    x1a, y1a, x1b, y1b = box1
    x2a, y2a, x2b, y2b = box2
    xa, ya = max(x1a, x2a), max(y1a, y2a)
    xb, yb = min(x1b, x2b), min(y1b, y2b)
    if xb <= xa or yb <= ya:
        return 0.0
    inter = (xb - xa) * (yb - ya)
    union = (x1b - x1a) * (y1b - y1a) + (x2b - x2a) * (y2b - y2a) - inter
    return inter / union if union > 0 else 0.0


def match_detections_to_bboxes(boxes_2d, bboxes_3d, colors, camera, min_iou=0.25):
    """[(corners_velo, rgb_color)] per detection whose best projected box beats min_iou (V4:140-183)."""
    pairs = []
    if not bboxes_3d or len(boxes_2d) == 0:
        return pairs
    proj = []
    for bbox in bboxes_3d:
        if "corners_cam0" not in bbox:
            proj.append(None)
            continue
        if "_bbox2d" in bbox:                                 # projected on the GPU by prepare_boxes
            proj.append(bbox["_bbox2d"])
            continue
        u, v, depth = camera.cam2image(np.array(bbox["corners_cam0"]).T)
        front = depth > 0
        proj.append([np.min(u[front]), np.min(v[front]), np.max(u[front]), np.max(v[front])] if front.sum() else None)
    for det_idx, box in enumerate(boxes_2d):
        x1, y1, x2, y2 = box
        best, best_idx = 0, -1
        for j, pb in enumerate(proj):
            if pb is None:
                continue
            iou = calculate_iou_2d([x1, y1, x2, y2], pb)
            if iou > best and iou > min_iou:
                best, best_idx = iou, j
        if best_idx >= 0 and "corners_velo" in bboxes_3d[best_idx]:
            c = colors[det_idx]
            pairs.append((np.array(bboxes_3d[best_idx]["corners_velo"]), np.array([c[2], c[1], c[0]]) / 255.0))
    return pairs


def _projected_box_info(bbox, camera):
    """V5's project_3d_bbox_to_2d (V5:215-252) for one box dict: None when no corner is in front."""
    if "_bbox2d" in bbox:                                   # projected on the GPU by prepare_boxes
        bb = bbox["_bbox2d"]
    else:
        u, v, depth = camera.cam2image(np.array(bbox["corners_cam0"]).T)
        front = depth > 0
        bb = [np.min(u[front]), np.min(v[front]), np.max(u[front]), np.max(v[front])] if np.any(front) else None
    if bb is None:
        return None
    x0, y0, x1, y1 = bb
    return {"bbox": [x0, y0, x1, y1], "center": [(x0 + x1) / 2, (y0 + y1) / 2], "size": [x1 - x0, y1 - y0],
            "area": (x1 - x0) * (y1 - y0)}


def calculate_matching_score(detection_info, bbox_3d_info, weight_iou=0.5, weight_center=0.3, weight_size=0.2):
    """0.5 IoU + 0.3 centre proximity + 0.2 area ratio (V5:277-304)."""
    iou = calculate_iou_2d(detection_info["bbox"], bbox_3d_info["bbox"])
    dist = np.linalg.norm(np.array(detection_info["center"]) - np.array(bbox_3d_info["center"]))
    center_score = max(0, 1 - dist / 1000)
    det_area = detection_info["size"][0] * detection_info["size"][1]
    box_area = bbox_3d_info["area"]
    size_ratio = min(det_area, box_area) / max(det_area, box_area) if det_area > 0 and box_area > 0 else 0
    total = weight_iou * iou + weight_center * center_score + weight_size * size_ratio
    return total, {"iou": iou, "center_score": center_score, "size_score": size_ratio, "total_score": total}


def improved_match_detections_to_bboxes(boxes_2d, bboxes_3d, mask_colors, camera, min_score_threshold=0.3,
                                        min_iou_threshold=0.15):
    """V5's score matrix + Hungarian assignment (V5:307-416): matched boxes in the detection's colour,
    then every unmatched box with 'corners_velo' in light grey.  Host scalars (D x B), scipy's solver."""
    from scipy.optimize import linear_sum_assignment
    matched = []
    if not bboxes_3d or len(boxes_2d) == 0:
        print("[INFO] No detections or 3D bounding boxes to match")
        return matched
    print(f"[INFO] Matching {len(boxes_2d)} 2D detections with {len(bboxes_3d)} 3D bboxes")
    dets = []
    for box in boxes_2d:
        if len(box) == 4:
            x1, y1, x2, y2 = box
            dets.append({"bbox": [x1, y1, x2, y2], "center": [(x1 + x2) / 2, (y1 + y2) / 2], "size": [x2 - x1, y2 - y1],
                         "area": (x2 - x1) * (y2 - y1)})
    infos, valid_idx = [], []
    for j, bbox in enumerate(bboxes_3d):
        info = _projected_box_info(bbox, camera) if "corners_cam0" in bbox else None
        if info is not None:
            infos.append(info)
            valid_idx.append(j)
    if not infos:
        print("[WARN] No valid 3D bbox projections found")
        return matched
    cost = np.zeros((len(dets), len(infos)))
    details = {}
    for i, d in enumerate(dets):
        for j, b in enumerate(infos):
            score, det = calculate_matching_score(d, b)
            cost[i, j] = 1 - score
            details[(i, j)] = det
    rows, cols = linear_sum_assignment(cost)
    pairs = []
    for i, j in zip(rows, cols):
        sc = details[(i, j)]
        pairs.append((i, j, sc["iou"], sc["center_score"], sc["size_score"], sc["total_score"],
                      sc["total_score"] >= min_score_threshold and sc["iou"] >= min_iou_threshold))
    return _report_matches(bboxes_3d, mask_colors, valid_idx, pairs)


def _report_matches(bboxes_3d, mask_colors, valid_idx, pairs):
    """V5's matcher from its assignment on (V5:366-416), for the scalar function and the batched ones alike: the returned list and
    every printed line.  pairs: the assigned pairs in row order as (detection, column, iou, center, size, total, accepted); valid_idx:
    the box of each column -- V5's columns are the boxes that have a projection."""
    matched, used = [], set()
    for i, j, iou, center, size, total, accepted in pairs:
        if accepted:
            orig = valid_idx[j]
            used.add(orig)
            bbox = bboxes_3d[orig]
            if "corners_velo" in bbox:
                if i < len(mask_colors):
                    c = mask_colors[i]
                    color = np.array([c[2], c[1], c[0]], dtype=float) / 255.0
                else:
                    color = np.array([1.0, 0.0, 0.0])
                matched.append((np.array(bbox["corners_velo"]), color))
                print(f"[INFO] Matched detection {i} with 3D bbox {orig}")
                print(f"        Scores - IoU: {iou:.3f}, Center: {center:.3f}, Size: {size:.3f}, Total: {total:.3f}")
            else:
                print(f"[WARN] No Velodyne corners found for bbox {orig}")
        else:
            print(f"[INFO] Rejected match det{i}-bbox{j}: score={total:.3f}, IoU={iou:.3f}")
    for i, bbox in enumerate(bboxes_3d):
        if i not in used and "corners_velo" in bbox:
            matched.append((np.array(bbox["corners_velo"]), [0.7, 0.7, 0.7]))
            print(f"[INFO] Added unmatched 3D bbox {i} in default color")
    return matched


# ---------------------------------------------------------------------------------------
# the same two matchers for a list of frames: the pair stage on the GPU (lpf_match_2d), one call per batch
# ---------------------------------------------------------------------------------------
def _match2d_dets(boxes_2d):
    """A frame's detections as a [D,4] array: float32 stays float32 (the detector's boxes.xyxy), anything else becomes float64."""
    if boxes_2d is None:
        return np.zeros((0, 4), np.float32)
    if type(boxes_2d).__module__.startswith("torch"):
        boxes_2d = boxes_2d.detach().cpu().numpy()
    d = np.asarray(boxes_2d)
    if d.size == 0:
        return np.zeros((0, 4), np.float32)
    if d.dtype != np.float32:
        d = d.astype(np.float64)
    if d.ndim != 2 or d.shape[1] != 4:
        raise ValueError("detections must be [D,4] (x1, y1, x2, y2), got %s" % (d.shape,))
    return d


def _match2d_rects(bboxes_per_frame, camera, ctx):
    """Per frame (bbox2d float64 [B,4], front int32 [B]) for EVERY dict of the frame's list, in order: prepare_boxes' '_bbox2d' /
    '_front' where a dict carries them, else the projection of its 'corners_cam0' -- all such boxes of the batch in ONE
    lpf_prepare_boxes call.  front = 0 (the matchers skip the box) for a dict without 'corners_cam0' or without a corner in front."""
    rects, todo, corners = [], [], []
    for f, boxes in enumerate(bboxes_per_frame):
        bb, fr = np.zeros((len(boxes), 4), np.float64), np.zeros(len(boxes), np.int32)
        for j, b in enumerate(boxes):
            if "corners_cam0" not in b:
                continue
            if "_bbox2d" in b:
                if b["_bbox2d"] is not None:
                    bb[j] = b["_bbox2d"]
                    fr[j] = b.get("_front", 8) or 8
            else:
                todo.append((f, j))
                corners.append(b["corners_cam0"])
        rects.append((bb, fr))
    if todo:
        ctx.ensure_intrinsics(camera.K, camera.width, camera.height)
        _, _, bb_all, fr_all = ctx.prepare_boxes(np.array(corners, np.float64).reshape(-1, 8, 3), np.eye(4))
        for (f, j), bb, fr in zip(todo, bb_all, fr_all):
            if fr > 0:
                rects[f][0][j], rects[f][1][j] = bb, fr
    return rects


def _per_frame_lists(*lists):
    """the per-frame arguments of a batched matcher as lists, one entry per frame in each"""
    lists = [list(x) for x in lists]
    if len({len(x) for x in lists}) > 1:
        raise ValueError("one entry per frame in each list")
    return lists


def _match2d_plan(boxes_2d_per_frame, bboxes_3d_per_frame, camera, device=0, ctx=None, rects=None):
    """What the batched matchers hand to the native calls: (live, dets, rects, ctx).  live[f]: the frame has detections and boxes (the
    matchers leave any other frame before they score); dets[f]: its detections (_match2d_dets), None for a dead frame; rects[f]: the
    (bbox2d, front) of every dict of its list, none for a dead frame -- the caller's ``rects`` where it has them already
    (lpf_box_views'), else _match2d_rects'.  Without a live frame rects and ctx are None: there is nothing to call."""
    live = [bool(b) and d is not None and len(d) > 0 for d, b in zip(boxes_2d_per_frame, bboxes_3d_per_frame)]
    dets = [_match2d_dets(d) if ok else None for d, ok in zip(boxes_2d_per_frame, live)]
    if not any(live):
        return live, dets, None, None
    ctx = ctx or get_context(device)
    if rects is None:
        rects = _match2d_rects([b if ok else [] for b, ok in zip(bboxes_3d_per_frame, live)], camera, ctx)
    else:
        rects = [r if ok else (np.zeros((0, 4), np.float64), np.zeros(0, np.int32)) for r, ok in zip(rects, live)]
    return live, dets, rects, ctx


def _dtype_groups(dets, rects, skip=()):
    """The frames of a plan that a native call takes -- those with detections and boxes, but for ``skip`` -- as (frames, dets, bbox2d,
    front) per detection dtype: a call's detections share one."""
    for dt in (np.float32, np.float64):
        idx = [f for f, d in enumerate(dets) if d is not None and d.dtype == dt and len(d) and len(rects[f][0]) and f not in skip]
        if idx:
            yield idx, [dets[f] for f in idx], [rects[f][0] for f in idx], [rects[f][1] for f in idx]


def _match2d_call(dets, rects, ctx, want, min_iou=0.25, skip=()):
    """ctx.match_2d over the frames that have detections and boxes, one call per detection dtype: per frame the dict of that frame's
    outputs, or None for a frame the matchers leave before they score anything (and for the frames of ``skip``)."""
    out = [None] * len(dets)
    for idx, d, bb, fr in _dtype_groups(dets, rects, skip):
        res = ctx.match_2d(d, bb, fr, min_iou=min_iou, want=want)
        for k, f in enumerate(idx):
            out[f] = {name: vals[k] for name, vals in res.items()}
    return out


def match_detections_frames(boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame, camera, min_iou=0.25, device=0, ctx=None):
    """match_detections_to_bboxes (V4:140-183) for a list of frames: per frame exactly the list that function returns, with the
    IoU of every (detection, box) pair and each detection's first strict maximum computed by ONE lpf_match_2d call for the batch.
    Box dicts without '_bbox2d' are projected for the whole batch by one lpf_prepare_boxes call."""
    boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame = _per_frame_lists(boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame)
    live, dets, rects, ctx = _match2d_plan(boxes_2d_per_frame, bboxes_3d_per_frame, camera, device, ctx)
    out = [[] for _ in live]
    if ctx is None:
        return out
    res = _match2d_call(dets, rects, ctx, ("best",), min_iou)
    for f, r in enumerate(res):
        if r is None:
            continue
        boxes, colors = bboxes_3d_per_frame[f], colors_per_frame[f]
        for det_idx, best_idx in enumerate(r["best_box"].tolist()):
            if best_idx >= 0 and "corners_velo" in boxes[best_idx]:
                c = colors[det_idx]
                out[f].append((np.array(boxes[best_idx]["corners_velo"]), np.array([c[2], c[1], c[0]]) / 255.0))
    return out


def _host_scores(dets, rects, ctx, skip=()):
    """The score matrices of a plan's frames (one lpf_match_2d call per detection dtype): per frame None (the matcher leaves before it
    scores; a frame of ``skip``) or (valid_idx, dict of [D, len(valid_idx)] matrices) -- V5's columns, the boxes with a projection."""
    out = []
    for f, r in enumerate(_match2d_call(dets, rects, ctx, ("iou", "center", "size", "total", "cost"), skip=skip)):
        if r is None:
            out.append(None)
            continue
        valid = np.flatnonzero(rects[f][1] > 0)
        out.append((valid.tolist(), {k: np.asarray(v)[:, valid] for k, v in r.items()}))
    return out


def _device_scores(dets, rects, ctx, min_score_threshold, min_iou_threshold):
    """_host_scores with the assignment made on the GPU as well (one lpf_assign_2d call per detection dtype): per frame None, or
    (valid_idx, pairs) with the assigned pairs in row order as (detection, compact column, iou, center, size, total, accepted) --
    what _improved_assign reads instead of the matrices.  A frame beyond LPF_ASSIGN_MAX detections or projected boxes gets
    _host_scores' entry: it is assigned on the host."""
    from ._native import LPF_ASSIGN_MAX, LpfContext
    over = {f for f, d in enumerate(dets) if d is not None and (len(d) > LPF_ASSIGN_MAX or int((rects[f][1] > 0).sum()) > LPF_ASSIGN_MAX)}
    out = [None] * len(dets)
    for idx, d, bb, fr in _dtype_groups(dets, rects, over):
        res = ctx.assign_2d(d, bb, fr, min_score_threshold=min_score_threshold, min_iou_threshold=min_iou_threshold)
        for k, f in enumerate(idx):
            if res["status"][k]:                             # (what scipy's solver raises for the frame's matrix)
                raise ValueError(LpfContext.ASSIGN_MESSAGES[int(res["status"][k])])
            valid = np.flatnonzero(rects[f][1] > 0)
            box = res["box_of_det"][k]
            rows = np.flatnonzero(box >= 0)
            cols = np.searchsorted(valid, box[rows])         # the box's rank among the projected ones: V5's column
            pairs = list(zip(rows.tolist(), cols.tolist(), *(res[n][k][rows].tolist() for n in ("iou", "center", "size", "total")),
                             (res["accepted"][k][rows] != 0).tolist()))
            out[f] = (valid.tolist(), pairs)
    if over:
        host = _host_scores(dets, rects, ctx, skip=set(range(len(dets))) - over)
        for f in over:
            out[f] = host[f]
    return out


def _assign_route(assign):
    if assign not in ("host", "device"):
        raise ValueError("assign is \"host\" (scipy's solver on the downloaded cost matrices) or \"device\" (lpf_assign_2d), got %r" % (assign,))
    return assign == "device"


def _improved_scores(boxes_2d_per_frame, bboxes_3d_per_frame, camera, min_score_threshold=0.3, min_iou_threshold=0.15, device=0, ctx=None,
                     rects=None, assign="host"):
    """What _improved_assign reads for each frame of a list, by either route: _host_scores' entries (assign="host") or _device_scores'
    (assign="device").  ``rects``: per frame the (bbox2d, front) of every dict of its list where the caller has them already."""
    to_device = _assign_route(assign)
    live, dets, rects, ctx = _match2d_plan(boxes_2d_per_frame, bboxes_3d_per_frame, camera, device, ctx, rects)
    if ctx is None:
        return [None] * len(live)
    if to_device:
        return _device_scores(dets, rects, ctx, min_score_threshold, min_iou_threshold)
    return _host_scores(dets, rects, ctx)


def _improved_assign(boxes_2d, bboxes_3d, mask_colors, scores, min_score_threshold=0.3, min_iou_threshold=0.15):
    """improved_match_detections_to_bboxes from its cost matrix on: the assignment, the thresholds, the returned list and every
    printed line, with the pair scores read from lpf_match_2d's matrices (``scores``: a frame's entry of _host_scores), or from
    the pairs lpf_assign_2d assigned (a frame's entry of _device_scores)."""
    if not bboxes_3d or boxes_2d is None or len(boxes_2d) == 0:
        print("[INFO] No detections or 3D bounding boxes to match")
        return []
    print(f"[INFO] Matching {len(boxes_2d)} 2D detections with {len(bboxes_3d)} 3D bboxes")
    valid_idx, m = scores
    if not valid_idx:
        print("[WARN] No valid 3D bbox projections found")
        return []
    if isinstance(m, list):                                 # assigned on the GPU
        pairs = m
    else:
        from scipy.optimize import linear_sum_assignment
        rows, cols = linear_sum_assignment(m["cost"])
        iou, center, size, total = m["iou"], m["center"], m["size"], m["total"]
        pairs = [(i, j, iou[i, j], center[i, j], size[i, j], total[i, j], total[i, j] >= min_score_threshold and iou[i, j] >= min_iou_threshold)
                 for i, j in zip(rows, cols)]
    return _report_matches(bboxes_3d, mask_colors, valid_idx, pairs)


def improved_match_detections_frames(boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame, camera, min_score_threshold=0.3,
                                     min_iou_threshold=0.15, device=0, ctx=None, assign="host"):
    """improved_match_detections_to_bboxes (V5:307-416) for a list of frames: per frame exactly the list that function returns and
    the same printed lines in the same order.  assign="host": the score of every (detection, box) pair of the batch comes from ONE
    lpf_match_2d call; the assignment is scipy's linear_sum_assignment on the downloaded cost matrix of the boxes that have a
    projection.  assign="device": scores, assignment and thresholds are ONE lpf_assign_2d call -- SciPy's assignment, ties included
    -- and a few words per detection come back instead of five [D,B] matrices; a frame beyond LPF_ASSIGN_MAX detections or
    projected boxes takes the host route."""
    boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame = _per_frame_lists(boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame)
    scores = _improved_scores(boxes_2d_per_frame, bboxes_3d_per_frame, camera, min_score_threshold, min_iou_threshold, device, ctx, assign=assign)
    return [_improved_assign(d, b, c, s, min_score_threshold, min_iou_threshold)
            for d, b, c, s in zip(boxes_2d_per_frame, bboxes_3d_per_frame, colors_per_frame, scores)]


def linear_sum_assignment_frames(costs, front=None, device=0, ctx=None):
    """scipy.optimize.linear_sum_assignment for a list of cost matrices in ONE native call (lpf_assign_costs): per frame (rows,
    cols) as SciPy returns them, its choice among equally good assignments included.  front: per frame [B] integers, a column with
    front <= 0 is left out (V5:337-341) and the columns keep their numbers.  ValueError with SciPy's message for a matrix with
    NaN or -inf entries, or without a complete assignment."""
    return (ctx or get_context(device)).assign_costs(costs, front)


# ---------------------------------------------------------------------------------------
# box-view helpers of secondtest.py / V5 / firsttest.py (8 corners per box: host scalars)
# ---------------------------------------------------------------------------------------
_HSV_SECTORS = ((0, 3, 1), (2, 0, 1), (1, 0, 3), (1, 2, 0), (3, 1, 0), (0, 1, 2))   # (r, g, b) picks from (value, p, q, t)


def generate_consistent_colors(n_objects):
    """BGR 0-255 tuples, golden-angle hues (V5:88-121): hue = i*137.508 mod 360,
    saturation 0.8 + 0.1*(i%3), value 0.8 + 0.2*(i%2)."""
    out = []
    for i in range(n_objects):
        hue = (i * 137.508) % 360
        sat, val = 0.8 + (i % 3) * 0.1, 0.8 + (i % 2) * 0.2
        sector = int(hue / 60) % 6
        frac = (hue / 60) - sector
        comp = (val, val * (1 - sat), val * (1 - frac * sat), val * (1 - (1 - frac) * sat))
        r, g, b = (comp[k] for k in _HSV_SECTORS[sector])
        out.append((int(b * 255), int(g * 255), int(r * 255)))
    return out


def project_3d_bbox_to_2d(bbox_3d, camera, detailed=True):
    """Image-plane box of the corners with depth > 0.  detailed=True: V5:215-252 /
    secondtest.py:215-252 -> ({'bbox','center','size','area','avg_depth'}, corners_cam0);
    detailed=False: firsttest.py:172-193 -> ([x_min, y_min, x_max, y_max], corners_cam0).
    (None, None) when nothing is in front of the camera or the dict has no corners."""
    try:
        corners = np.array(bbox_3d["corners_cam0"])
        u, v, depth = camera.cam2image(corners.T)
        front = depth > 0
        if np.any(front):
            x0, x1 = np.min(u[front]), np.max(u[front])
            y0, y1 = np.min(v[front]), np.max(v[front])
            if not detailed:
                return [x0, y0, x1, y1], corners
            return {"bbox": [x0, y0, x1, y1], "center": [(x0 + x1) / 2, (y0 + y1) / 2], "size": [x1 - x0, y1 - y0],
                    "area": (x1 - x0) * (y1 - y0), "avg_depth": np.mean(depth[front])}, corners
    except Exception as e:
        print(f"[ERROR] Failed to project 3D bbox: {e}")
    return None, None


def is_bbox_in_camera_view(bbox_3d, camera, min_points_in_view=4, depth_range=(0.1, 100)):
    """(keep, info) of secondtest.py:277-359.  Corners count when depth lies in the closed
    depth_range; a box is dropped when none do ('all_behind_camera'), when fewer than
    min_points_in_view corners are inside the image AND the corners' pixel box misses the image
    ('no_intersection'), or when that pixel box is under 100 px^2 ('too_small')."""
    try:
        if "corners_cam0" not in bbox_3d:
            return False, {"reason": "no_corners"}
        u, v, depth = camera.cam2image(np.array(bbox_3d["corners_cam0"]).T)
        near = (depth >= depth_range[0]) & (depth <= depth_range[1])
        n_near = np.sum(near)
        if n_near == 0:
            return False, {"reason": "all_behind_camera", "depths": depth.tolist()}
        in_view = np.sum(near & (u >= 0) & (u < camera.width) & (v >= 0) & (v < camera.height))
        un, vn = u[near], v[near]
        if in_view < min_points_in_view:
            x0, x1, y0, y1 = np.min(un), np.max(un), np.min(vn), np.max(vn)
            if x1 < 0 or x0 >= camera.width or y1 < 0 or y0 >= camera.height:
                return False, {"reason": "no_intersection", "corners_in_view": in_view, "bbox_2d": [x0, y0, x1, y1]}
        if n_near >= 2:
            u_range, v_range = np.max(un) - np.min(un), np.max(vn) - np.min(vn)
            if u_range * v_range < 100:
                return False, {"reason": "too_small", "projected_area": u_range * v_range,
                               "u_range": u_range, "v_range": v_range}
        return True, {"reason": "valid", "corners_in_view": in_view, "corners_with_valid_depth": n_near,
                      "avg_depth": np.mean(depth[near]) if n_near > 0 else 0}
    except Exception as e:
        print(f"[ERROR] Error checking bbox visibility: {e}")
        return False, {"reason": "error", "error": str(e)}


def filter_bboxes_in_camera_view(bboxes_3d, camera, verbose=True):
    """(kept boxes in order, {'total','kept','filtered','filter_reasons'}) -- secondtest.py:362-419."""
    if not bboxes_3d:
        return [], {"total": 0, "kept": 0, "filtered": 0, "filter_reasons": {}}
    kept, reasons = [], {}
    for i, bbox in enumerate(bboxes_3d):
        ok, info = is_bbox_in_camera_view(bbox, camera)
        if ok:
            kept.append(bbox)
            if verbose:
                print(f"[INFO] Kept bbox {i}: {info['corners_in_view']} corners in view, "
                      f"avg depth: {info.get('avg_depth', 0):.2f}m")
            continue
        why = info["reason"]
        reasons[why] = reasons.get(why, 0) + 1
        if verbose:
            print(f"[INFO] Filtered bbox {i}: {why}")
            if why == "all_behind_camera" and info.get("depths"):
                print(f"        Depths: min={min(info['depths']):.2f}, max={max(info['depths']):.2f}")
            elif why == "no_intersection":
                print(f"        2D bbox: {info.get('bbox_2d', [])}")
            elif why == "too_small":
                print(f"        Projected area: {info.get('projected_area', 0):.1f} pixels")
    stats = {"total": len(bboxes_3d), "kept": len(kept), "filtered": len(bboxes_3d) - len(kept), "filter_reasons": reasons}
    if verbose:
        print(f"\n[STATS] BBox Filtering Results:")
        print(f"        Total: {stats['total']}")
        print(f"        Kept: {stats['kept']}")
        print(f"        Filtered: {stats['filtered']}")
        print(f"        Filter reasons: {stats['filter_reasons']}")
    return kept, stats


# ---------------------------------------------------------------------------------------
# the same box-view helpers for a list of frames: every box of the batch in ONE lpf_box_views call
# ---------------------------------------------------------------------------------------
_VIEW_REASONS = ("valid", "no_corners", "all_behind_camera", "no_intersection", "too_small", "error")
_NO_CORNERS, _SCALAR = -1, -2


def _view_batch(bboxes_per_frame):
    """The boxes of a batch as lpf_box_views takes them: (slots, corners float64 [Btot,8,3], box_off int64 [F+1]).  slots[f][i] is
    the position of frame f's dict i among the call's boxes, _NO_CORNERS for a dict without 'corners_cam0' (the host's no_corners),
    or _SCALAR for one whose corners are not 8 x 3 numbers: the scalar function decides about it, as it always has."""
    slots, parts, off = [], [], [0]
    for boxes in bboxes_per_frame:
        have = [i for i, b in enumerate(boxes) if "corners_cam0" in b]
        slot = [_NO_CORNERS] * len(boxes)
        arr = None
        try:
            arr = np.array([boxes[i]["corners_cam0"] for i in have]) if have else np.zeros((0, 8, 3))
        except ValueError:                                  # ragged
            pass
        if arr is not None and arr.shape == (len(have), 8, 3) and arr.dtype.kind in "fiu":
            for k, i in enumerate(have):
                slot[i] = off[-1] + k
            parts.append(arr.astype(np.float64, copy=False))
            n = len(have)
        else:                                               # some dict of the frame is odd: look at each
            n = 0
            for i in have:
                try:
                    c = np.array(boxes[i]["corners_cam0"])
                except ValueError:
                    c = None
                if c is not None and c.shape == (8, 3) and c.dtype.kind in "fiu":
                    slot[i] = off[-1] + n
                    parts.append(c.astype(np.float64).reshape(1, 8, 3))
                    n += 1
                else:
                    slot[i] = _SCALAR
        slots.append(slot)
        off.append(off[-1] + n)
    corners = np.concatenate(parts) if parts else np.zeros((0, 8, 3), np.float64)
    return slots, np.ascontiguousarray(corners.reshape(-1, 8, 3)), np.array(off, np.int64)


def _view_call(bboxes_per_frame, camera, want, device=0, ctx=None, T_cam_to_velo=None):
    """(slots, corners, results) of ONE lpf_box_views call over every box of the batch that has 8 x 3 corners; results are host lists
    (``tolist()`` once per array: per box it would cost more than the kernel), None when the batch has no such box."""
    slots, corners, off = _view_batch(bboxes_per_frame)
    if not len(corners):
        return slots, corners, None
    ctx = ctx or get_context(device)
    ctx.ensure_intrinsics(camera.K, camera.width, camera.height)
    res = ctx.box_views(corners, off, T_cam_to_velo=T_cam_to_velo, want=want)
    return slots, corners, res


def _filter_frame(boxes, slot, res, depth, camera, verbose, kept_slots=None):
    """filter_bboxes_in_camera_view for one frame from the batch's results: its (kept, stats) and printed lines (kept_slots: a list
    that receives the kept boxes' slots)"""
    if not boxes:
        return [], {"total": 0, "kept": 0, "filtered": 0, "filter_reasons": {}}
    kept, reasons = [], {}
    for i, bbox in enumerate(boxes):
        j = slot[i]
        if j == _SCALAR:
            ok, info = is_bbox_in_camera_view(bbox, camera)
            why = info["reason"]
        elif j == _NO_CORNERS:
            ok, info, why = False, None, "no_corners"
        else:
            ok, info, why = bool(res["keep"][j]), None, _VIEW_REASONS[res["reason"][j]]
        if ok:
            kept.append(bbox)
            if kept_slots is not None:
                kept_slots.append(j)
            if verbose:
                n, avg = (info["corners_in_view"], info.get("avg_depth", 0)) if info else (res["corners_in_view"][j], res["avg_depth"][j])
                print(f"[INFO] Kept bbox {i}: {n} corners in view, avg depth: {avg:.2f}m")
            continue
        reasons[why] = reasons.get(why, 0) + 1
        if verbose:
            print(f"[INFO] Filtered bbox {i}: {why}")
            if why == "all_behind_camera":
                d = info["depths"] if info else depth[j]
                if d:
                    print(f"        Depths: min={min(d):.2f}, max={max(d):.2f}")
            elif why == "no_intersection":
                bb = info.get("bbox_2d", []) if info else [np.int64(x) for x in res["near_bbox2d"][j]]
                print(f"        2D bbox: {bb}")
            elif why == "too_small":
                if info:
                    area = info.get("projected_area", 0)
                else:
                    x0, y0, x1, y1 = (np.int64(x) for x in res["near_bbox2d"][j])
                    area = (x1 - x0) * (y1 - y0)
                print(f"        Projected area: {area:.1f} pixels")
    stats = {"total": len(boxes), "kept": len(kept), "filtered": len(boxes) - len(kept), "filter_reasons": reasons}
    if verbose:
        print(f"\n[STATS] BBox Filtering Results:")
        print(f"        Total: {stats['total']}")
        print(f"        Kept: {stats['kept']}")
        print(f"        Filtered: {stats['filtered']}")
        print(f"        Filter reasons: {stats['filter_reasons']}")
    return kept, stats


def _filter_setup(bboxes_per_frame, camera, verbose, device, ctx, extra=(), T_cam_to_velo=None):
    """The one lpf_box_views call of the batched filter: (slots, results as host lists or None, the depths of the boxes behind the
    camera -- what the verbose lines print of them -- by position, raw results)"""
    want = ("keep", "reason") + (("corners_in_view", "avg_depth", "near_bbox2d") if verbose else ()) + tuple(extra)
    slots, corners, raw = _view_call(bboxes_per_frame, camera, want, device, ctx, T_cam_to_velo)
    if raw is None:
        return slots, None, {}, None
    res = {k: np.asarray(raw[k]).tolist() for k in want if k not in extra}
    depth = {}
    if verbose:
        behind = np.flatnonzero(np.asarray(raw["reason"]) == 2)
        if len(behind):
            d = camera.cam2image(corners[behind].transpose(0, 2, 1))[2].tolist()
            depth = dict(zip(behind.tolist(), d))
    return slots, res, depth, raw


def filter_bboxes_in_camera_view_frames(bboxes_per_frame, camera, verbose=True, device=0, ctx=None):
    """filter_bboxes_in_camera_view (secondtest.py:362-419) for a list of frames: per frame exactly the (kept, stats) that function
    returns -- ``kept`` holds the same dict objects, the ``filter_reasons`` keys come in first-seen order -- and the same printed
    lines in the same order, frame by frame.  Every box of the batch is judged by ONE lpf_box_views call; a dict without
    'corners_cam0' is 'no_corners' on the host and is left out of the call."""
    bboxes_per_frame = [list(b) if b else [] for b in bboxes_per_frame]
    slots, res, depth, _ = _filter_setup(bboxes_per_frame, camera, verbose, device, ctx)
    return [_filter_frame(boxes, slot, res, depth, camera, verbose) for boxes, slot in zip(bboxes_per_frame, slots)]


def project_3d_bboxes_to_2d_frames(bboxes_per_frame, camera, detailed=True, device=0, ctx=None):
    """project_3d_bbox_to_2d (V5:215-252; detailed=False: firsttest.py:172-193) for a list of frames: per frame the list of
    (info, corners) that function returns per box, with the same value types (np.int64 pixels, float centre, np.float64 avg_depth).
    Every box of the batch is projected by ONE lpf_box_views call."""
    bboxes_per_frame = [list(b) if b else [] for b in bboxes_per_frame]
    want = ("front", "bbox2d") + (("front_avg_depth",) if detailed else ())
    slots, corners, res = _view_call(bboxes_per_frame, camera, want, device, ctx)
    if res is not None:
        front = np.asarray(res["front"]).tolist()
        bb = np.where(np.asarray(res["front"])[:, None] > 0, np.asarray(res["bbox2d"]), 0.0).astype(np.int64)
        avg = np.asarray(res["front_avg_depth"]) if detailed else None
    out = []
    for boxes, slot in zip(bboxes_per_frame, slots):
        rows = []
        for bbox, j in zip(boxes, slot):
            if j < 0:                                       # no corners, or odd ones: the scalar function's answer and printed line
                rows.append(project_3d_bbox_to_2d(bbox, camera, detailed))
            elif front[j] == 0:
                rows.append((None, None))
            else:
                x0, y0, x1, y1 = bb[j]
                c = np.array(bbox["corners_cam0"])
                if not detailed:
                    rows.append(([x0, y0, x1, y1], c))
                else:
                    rows.append(({"bbox": [x0, y0, x1, y1], "center": [(x0 + x1) / 2, (y0 + y1) / 2], "size": [x1 - x0, y1 - y0],
                                  "area": (x1 - x0) * (y1 - y0), "avg_depth": avg[j]}, c))
        out.append(rows)
    return out


def secondtest_match_frames(boxes_2d_per_frame, bboxes_raw_per_frame, colors_per_frame, camera, TrVeloToCam, verbose=True,
                            min_score_threshold=0.3, min_iou_threshold=0.15, device=0, ctx=None, assign="host"):
    """secondtest.py:599-611 and :703 for a list of frames: filter_bboxes_in_camera_view, then transform_bboxes_to_velodyne on the
    kept boxes, then improved_match_detections_to_bboxes.  Per frame (matched_pairs, filter_stats, bboxes_3d); the results and the
    printed lines equal the scalar composition of the package's three functions, and -- as there -- the kept dicts gain
    'corners_velo' in place and nothing else.  Two native calls per batch: lpf_box_views, whose front bbox2d / front of the kept
    boxes and whose corners_velo feed the matcher, and lpf_match_2d -- or, with assign="device", lpf_assign_2d, which assigns on the
    GPU as well (improved_match_detections_frames)."""
    _assign_route(assign)                                  # (refused here, before anything is filtered or printed)
    boxes_2d_per_frame, bboxes_raw_per_frame, colors_per_frame = _per_frame_lists(boxes_2d_per_frame, bboxes_raw_per_frame, colors_per_frame)
    bboxes_raw_per_frame = [list(b) if b else [] for b in bboxes_raw_per_frame]
    slots, res, depth, raw = _filter_setup(bboxes_raw_per_frame, camera, verbose, device, ctx, ("front", "bbox2d", "corners_velo"),
                                           np.linalg.inv(TrVeloToCam))
    filtered, lines, rects = [], [], []
    for boxes, slot in zip(bboxes_raw_per_frame, slots):
        idx = []
        with contextlib.redirect_stdout(io.StringIO()) as buf:                 # (a frame's lines are printed below, before its matcher's)
            kept, stats = _filter_frame(boxes, slot, res, depth, camera, verbose, idx)
        filtered.append((kept, stats))
        lines.append(buf.getvalue())
        bb, fr = np.zeros((len(kept), 4), np.float64), np.zeros(len(kept), np.int32)
        odd = [k for k, j in enumerate(idx) if j < 0]
        if odd:                                             # kept by the scalar function: transformed and projected as it always was
            transform_bboxes_to_velodyne([kept[k] for k in odd], TrVeloToCam)
        for k, j in enumerate(idx):
            if j >= 0:
                kept[k]["corners_velo"] = raw["corners_velo"][j].tolist()
                fr[k] = raw["front"][j]
                if fr[k] > 0:
                    bb[k] = raw["bbox2d"][j]
            else:
                info = _projected_box_info({"corners_cam0": kept[k]["corners_cam0"]}, camera)
                if info is not None:
                    bb[k], fr[k] = info["bbox"], 8
        rects.append((bb, fr))
    kept_per_frame = [k for k, _ in filtered]
    scores = _improved_scores(boxes_2d_per_frame, kept_per_frame, camera, min_score_threshold, min_iou_threshold, device, ctx, rects, assign)
    out = []
    for f, (kept, stats) in enumerate(filtered):
        sys.stdout.write(lines[f])
        matched = _improved_assign(boxes_2d_per_frame[f], kept, colors_per_frame[f], scores[f], min_score_threshold, min_iou_threshold)
        out.append((matched, stats, kept))
    return out


# ---------------------------------------------------------------------------------------
# exclusive labelling of Same_color.py:113-131 (first matching mask wins)
# ---------------------------------------------------------------------------------------
def _same_color_canvas(masks, camera):
    """Same_color.py:124 indexes every mask AT ITS OWN SIZE -- ``y < mask.shape[0] and x < mask.shape[1] and mask[y, x] > 0.5``, no
    resize -- so a mask that does not arrive at the camera's size counts in the pixels the two sizes share and nowhere else: the mask
    cropped / zero-padded to [H, W].  Masks at camera size (and GPU tensors at camera size) pass through."""
    H, W = camera.height, camera.width
    if _is_device_tensor(masks):
        import torch
        if masks.ndim != 3:
            raise ValueError("device masks must be [M,h,w]")
        if tuple(masks.shape[1:]) == (H, W):
            return _mask_stack(masks, camera)[0]
        src = masks if masks.dtype in (torch.float32, torch.uint8) else masks.to(torch.float32)
        canvas = torch.zeros((masks.shape[0], H, W), dtype=src.dtype, device=masks.device)
        h, w = min(H, masks.shape[1]), min(W, masks.shape[2])
        canvas[:, :h, :w] = src[:, :h, :w]
        return canvas
    planes = [np.asarray(mk) for mk in masks] if not isinstance(masks, np.ndarray) else list(masks)
    if not planes:
        return np.zeros((0, H, W), np.uint8)
    if all(pl.shape == (H, W) for pl in planes):
        return _mask_stack(np.stack(planes), camera)[0]
    flt = any(pl.dtype.kind == "f" for pl in planes)
    canvas = np.zeros((len(planes), H, W), np.float32 if flt else np.uint8)
    for i, pl in enumerate(planes):                          # (the reference's list may hold masks of different sizes)
        if pl.ndim != 2:
            raise ValueError("masks must be a list of [h,w] arrays or an [M,h,w] array")
        h, w = min(H, pl.shape[0]), min(W, pl.shape[1])
        canvas[i, :h, :w] = pl[:h, :w]
    return canvas


def label_points_first_match(points, TrVeloToRect, camera, masks, mask_colors=None, depth_max=30.0, device=0):
    """Same_color.py's per-point double loop as one fused GPU pass.  Returns a dict:
    ``car_idx`` (indices into points of valid points that lie in some mask, ascending),
    ``car_mask`` (the FIRST mask each of them matched, ``mask[y, x] > 0.5``), ``background_idx``
    (valid points in no mask), and ``colored_points`` / ``colored_colors`` / ``full_points`` as the
    reference accumulates them (colors = mask_colors[i] / 255.0 when mask_colors is given)."""
    p = _f32_points(points).reshape(-1, 4)
    m = _same_color_canvas(masks, camera)
    if m.shape[0] > LPF_MAX_MASKS:
        raise ValueError("at most %d masks per frame" % LPF_MAX_MASKS)
    ctx = get_context(device)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    ctx.set_masks(m, binarize="gt0.5")
    ctx.clear_boxes()
    r = ctx.run(p, want_uv=False)
    ctx.clear_masks()
    vidx = r["valid_idx"]
    bits = r["label_bits"][vidx]
    hit = bits != 0
    low = bits[hit] & (~bits[hit] + np.uint32(1))                       # lowest set bit = first mask in list order
    first = np.log2(low.astype(np.float64)).astype(np.int64) if low.size else np.zeros(0, np.int64)
    out = {"car_idx": vidx[hit], "car_mask": first, "background_idx": vidx[~hit],
           "colored_points": p[vidx[hit], :3], "full_points": p[vidx[~hit], :3]}
    if mask_colors is not None:
        table = np.array([np.array(c) / 255.0 for c in mask_colors], np.float64).reshape(-1, 3)
        out["colored_colors"] = table[first]
    return out


def _first_match_planes(masks):
    """One frame's masks for first_match_frames: (a GPU tensor [M,h,w], or a list of 2-D host arrays; is any of them float)."""
    if masks is None:
        return [], False
    if _is_device_tensor(masks):
        if masks.dim() != 3:
            raise ValueError("device masks must be [M,h,w], got %s" % (tuple(masks.shape),))
        return masks, str(masks.dtype) not in ("torch.uint8", "torch.bool")
    planes = [np.asarray(mk) for mk in masks]
    for pl in planes:
        if pl.ndim != 2:
            raise ValueError("masks must be a list of [h,w] arrays or an [M,h,w] array, got a mask of shape %s" % (pl.shape,))
    return planes, any(pl.dtype.kind == "f" for pl in planes)


def _first_match_masks(frames, camera):
    """The frames' masks as ONE [F,M,mh,mw] batch for lpf_first_match (M = the most masks of a frame; the others pad with empty
    planes) and each frame's own count.  Masks that all share one size go down AT THAT SIZE, whatever the camera's -- Same_color.py:125
    reads every mask at its own size -- and a ragged list falls back to _same_color_canvas (each mask cropped / zero-padded to the
    camera's size, which holds the same members).  float masks are read as ``mask > 0.5``, the others as ``> 0``; a batch that mixes
    them goes as float32.  GPU tensors stay on the GPU."""
    per = [_first_match_planes(f.masks) for f in frames]
    sizes = {tuple(pl.shape[-2:]) for planes, _ in per for pl in planes}
    if len(sizes) > 1:                                      # ragged: the canvas at the camera's size
        per = [(_same_color_canvas(f.masks, camera), flt) if len(planes) else (planes, flt) for f, (planes, flt) in zip(frames, per)]
        sizes = {(int(camera.height), int(camera.width))}
    return _padded_mask_batch([planes for planes, _ in per], [flt for _, flt in per], sizes.pop() if sizes else (1, 1), lambda a: a > 0)[:2]


def _padded_mask_batch(stacks, floats, size, member):
    """The frames' masks as ONE [F,M,h,w] batch -- M = the most masks of a frame, the others pad with empty planes -- behind
    _first_match_masks and _depth_map_masks: (batch, each frame's own count, is the batch float32).  stacks: per frame an [M_f,h,w]
    NumPy array or GPU tensor of ``size`` = (h, w), a list of [h,w] host planes (never stacked on the host: 135 MB per frame at 256
    masks), or anything empty; floats: is that frame's stack read as float (``> 0.5`` on the GPU).  A batch that mixes float and other masks goes as float32, one without float masks as uint8 under ``member``, the caller's
    rule for them (``> 0`` or ``!= 0``: they differ for negative integers).  GPU tensors stay on the GPU: the batch is made there."""
    Ms = [len(m) for m in stacks]
    M = max(Ms) if Ms else 0
    flt = any(f for m, f in zip(stacks, floats) if len(m))
    on_gpu = [m for m in stacks if _is_device_tensor(m) and len(m)]
    if on_gpu:
        import torch
        dev = on_gpu[0].device
        batch = torch.zeros((len(stacks), M) + tuple(size), dtype=torch.float32 if flt else torch.uint8, device=dev)
        for i, m in enumerate(stacks):
            if len(m):
                t = (m if _is_device_tensor(m) else torch.from_numpy(np.ascontiguousarray(m))).to(dev)
                batch[i, :len(m)].copy_(t if flt else member(t))
        return batch, Ms, flt
    batch = np.zeros((len(stacks), M) + tuple(size), np.float32 if flt else np.uint8)
    for i, m in enumerate(stacks):
        for j, pl in enumerate(m):                            # plane by plane: the temporaries stay small
            batch[i, j] = pl if flt else member(pl)
    return batch, Ms, flt


def _mask_group(batch, rles, g):
    """Masks g .. g + 255 of every frame, as first_match and depth_maps take them: the frames' RleMasks sliced, or (rles None) those
    planes of the dense batch, contiguous."""
    if rles is not None:
        return [r[g:g + LPF_MAX_MASKS_WIDE] for r in rles]
    part = batch[:, g:g + LPF_MAX_MASKS_WIDE]
    return part.contiguous() if _is_device_tensor(part) else np.ascontiguousarray(part)


def _first_match_rle_masks(frames):
    """Each frame's RleMasks when the batch's masks come in run-length form, None when no frame's do: _compact_frame_masks' rules, with
    the size the frames' RleMasks share in the camera's place -- first_match reads masks at their own size.  ValueError: RleMasks of
    differing sizes, and what _compact_frame_masks refuses."""
    sizes = sorted({tuple(f.masks.shape[1:]) for f in frames if isinstance(f.masks, RleMasks)})
    if not sizes:
        return None
    if len(sizes) > 1:
        raise ValueError("first_match_frames: the frames' RleMasks have differing sizes (H, W) = %s: one size per batch (runs are not "
                         "resized: decode with .to_dense())" % (sizes,))
    return _compact_frame_masks(frames, None, ("rle",), size=sizes[0])[1]


def first_match_frames(frames, TrVeloToRect, camera, depth_max=30.0, mask_colors=None, device=0, ctx=None):
    """Same_color.py:113-132 for a list of FrameInputs: one native call (lpf_first_match) per group of up to 256 masks for the whole
    batch, no limit on the masks of a frame.  Per frame the dict label_points_first_match returns -- ``car_idx``, ``car_mask``,
    ``background_idx``, ``colored_points``, ``colored_colors``, ``full_points`` -- plus ``mask_count`` (int64, the points whose first
    mask is m, per mask of the frame).  mask_colors: one list of colours per frame (colored_colors = colour / 255.0, as the script
    computes it); None takes each frame's ``colors``.  Points: host arrays, Scans of the read-ahead reader or GPU tensors; masks: a
    list, an array or a GPU tensor [M,h,w] AT THEIR OWN SIZE, float (> 0.5) or uint8 / bool (nonzero), or ``rle.RleMasks`` (every
    frame of the batch, a frame without masks aside, all of one size: they go down as runs, nothing dense is made); frames may differ
    in their mask counts.  A later group can only claim points no earlier group claimed: with more than 256 masks the groups' dense codes are
    merged and the lists are made from the merged codes.  The depth window is (0, depth_max)."""
    frames = list(frames)
    if not frames:
        return []
    if mask_colors is not None and len(mask_colors) != len(frames):
        raise ValueError("mask_colors: one list of colours per frame (%d frames, %d lists)" % (len(frames), len(mask_colors)))
    rles = _first_match_rle_masks(frames)
    if rles is not None:                                    # run-length masks: the runs go down as they are (lpf_first_match_rle)
        batch, Ms = None, [len(r) for r in rles]
        F, M = len(frames), max(Ms)
    else:
        batch, Ms = _first_match_masks(frames, camera)
        F, M = len(frames), int(batch.shape[1])
    table = np.zeros((F, M, 3), np.float64)
    for f, fr in enumerate(frames):
        cols = fr.colors if mask_colors is None else mask_colors[f]
        if len(cols) < Ms[f]:
            raise ValueError("frame %s: %d masks, %d colours" % (fr.frame, Ms[f], len(cols)))
        for i in range(Ms[f]):
            table[f, i] = np.array(cols[i]) / 255.0
    ctx = ctx or get_context(device)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    gpu = _is_device_tensor(batch)

    def host(a):
        return a.cpu().numpy() if _is_device_tensor(a) else a

    def colours(part):
        if not gpu:
            return part
        import torch
        return torch.from_numpy(np.ascontiguousarray(part)).to(batch.device)

    staged = ctx.stage_points([f.points for f in frames])
    off = staged[0]
    out = []
    if M <= LPF_MAX_MASKS_WIDE:                             # one call: the lists as the GPU made them
        r = ctx.first_match(None, batch if rles is None else rles, colours(table), want=("car_idx", "car_mask", "car_xyz", "car_rgb", "bg_idx", "bg_xyz", "mask_count"),
                            staged=staged)
        r = {k: host(v) for k, v in r.items()}
        for f in range(F):
            a, nc, nb = int(off[f]), int(r["n_car"][f]), int(r["n_bg"][f])
            out.append({"car_idx": r["car_idx"][a:a + nc].copy(), "car_mask": r["car_mask"][a:a + nc].astype(np.int64),
                        "background_idx": r["bg_idx"][a:a + nb].copy(), "colored_points": r["car_xyz"][a:a + nc].copy(),
                        "full_points": r["bg_xyz"][a:a + nb].copy(), "colored_colors": r["car_rgb"][a:a + nc].copy(),
                        "mask_count": r["mask_count"][f, :Ms[f]].copy()})
        return out
    code = None
    for g in range(0, M, LPF_MAX_MASKS_WIDE):               # groups of 256 masks, merged on the dense codes
        cur = host(ctx.first_match(None, _mask_group(batch, rles, g), want=("first_mask",), staged=staged)["first_mask"])
        code = cur if code is None else np.where((code == -1) & (cur >= 0), cur + np.int32(g), code)
    for f, fr in enumerate(frames):
        cf = code[int(off[f]):int(off[f + 1])]
        car, bg = np.flatnonzero(cf >= 0), np.flatnonzero(cf == -1)
        first = cf[car].astype(np.int64)
        p = fr.points.points if isinstance(fr.points, Scan) else host(fr.points)
        out.append({"car_idx": car, "car_mask": first, "background_idx": bg, "colored_points": p[car, :3], "full_points": p[bg, :3],
                    "colored_colors": table[f][first], "mask_count": np.bincount(first, minlength=Ms[f]).astype(np.int64)})
    return out


def process_frames_same_color(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None, frames=None, depth_max=30.0,
                              device=0):
    """Same_color.projectVeloToImage's frame loop (Same_color.py:80-138) without the Open3D window: yields ``(frame, result)`` with
    result first_match_frames' dict for every frame that has a valid LiDAR point.  Scans are read in order by the native read-ahead
    reader.  ``segmenter(image) -> (img, masks, mask_colors)`` is the segmentation stage (it stays outside this package).  The
    script's ``[INFO]`` / ``[DEBUG]`` / ``[WARN]`` / ``[ERROR]`` lines are printed verbatim: a scan that cannot be read and a missing
    image skip the frame (:88-90, :102-104), ``masks is None`` shows the plain cloud (:109-111), a frame without a valid point is
    skipped with the script's warning (:136-138)."""
    if segmenter is None:
        raise ValueError("process_frames_same_color needs the segmentation callable (YOLO stays outside this package)")
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    sequence, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    todo = velo.available_frames() if frames is None else list(frames)
    paths = [os.path.join(velo.raw3DPcdPath, "%010d.bin" % f) for f in todo]
    print(f"[INFO] Found {len(todo)} Velodyne frames.")
    if not paths:
        return
    ctx = get_context(device)
    sizes = [os.path.getsize(p) // 16 for p in paths if os.path.isfile(p)]
    with ScanReader(ctx, paths, n_buffers=3, max_points=max(sizes + [1])) as reader:
        for frame_idx, frame in enumerate(todo):
            print(f"\n[INFO] Processing frame {frame} ({frame_idx + 1}/{len(todo)})...")
            try:
                scan = next(reader)
                print(f"[DEBUG] Loaded {len(scan.points)} points from frame {frame}")
            except Exception as e:
                print(f"[ERROR] Failed to load velodyne data for frame {frame}: {e}")
                continue
            image_path = os.path.join(root, "data_2d_raw", sequence, f"image_{cam_id:02d}",
                                      "data_rect" if cam_id in [0, 1] else "data_rgb", "%010d.png" % frame)
            if not os.path.isfile(image_path):
                print(f"[WARN] Image not found: {image_path}")
                continue
            _, masks, colors = segmenter(image_loader(image_path) if image_loader else image_path)[:3]
            if masks is None:
                print(f"[INFO] No cars detected in frame {frame}, showing plain cloud.")
                masks, colors = [], []
            r = first_match_frames([FrameInputs(frame, scan, masks, colors=colors)], velo_to_rect, camera, depth_max, None, device, ctx)[0]
            n_car, n_bg = len(r["car_idx"]), len(r["background_idx"])
            print(f"[DEBUG] Frame {frame}: {n_car + n_bg} points passed validation filter")
            print(f"[DEBUG] Frame {frame}: {n_car} car points, {n_bg} background points")
            if not n_car and not n_bg:
                print(f"[WARN] No valid LiDAR points in frame {frame}")
                continue
            yield frame, r


# ---------------------------------------------------------------------------------------
# reporting (V3:431-468, cvs_erosion.py:232-295)
# ---------------------------------------------------------------------------------------
def print_summary_statistics(car_statistics):
    if not car_statistics:
        print("\nNo car statistics to display.")
        return
    print(f"\n{'=' * 60}")
    print(f"{'SUMMARY STATISTICS':^60}")
    print(f"{'=' * 60}")
    matched = [s for s in car_statistics if s["matched_bbox_id"] >= 0]
    print(f"Total cars detected: {len(car_statistics)}")
    print(f"Successfully matched: {len(matched)}")
    print(f"Unmatched: {len(car_statistics) - len(matched)}")
    if matched:
        print(f"\n{'Car ID':<8} {'BBox ID':<8} {'Total':<8} {'Inside':<8} {'Outside':<8} {'Inside %':<10}")
        print("-" * 60)
        for s in matched:
            print(f"{s['car_id']:<8} {s['matched_bbox_id']:<8} {s['total_points']:<8} {s['points_inside_bbox']:<8} "
                  f"{s['points_outside_bbox']:<8} {s['inside_percentage']:<10.1f}")
        tp = sum(s["total_points"] for s in matched)
        ti = sum(s["points_inside_bbox"] for s in matched)
        to = sum(s["points_outside_bbox"] for s in matched)
        avg = (ti / tp * 100) if tp > 0 else 0
        print("-" * 60)
        print(f"{'TOTAL':<8} {'':<8} {tp:<8} {ti:<8} {to:<8} {avg:<10.1f}")


CSV_COLUMNS = ("frame", "car_id", "matched_bbox_id", "total_points", "points_inside_bbox", "points_outside_bbox",
               "inside_percentage", "outside_percentage", "is_matched", "timestamp")


def csv_rows(car_statistics, frame_number, timestamp=None):
    """The rows append_to_master_csv writes (cvs_erosion.py:243-255)."""
    ts = timestamp if timestamp is not None else datetime.now().isoformat()
    return [{"frame": frame_number, "car_id": s["car_id"], "matched_bbox_id": s["matched_bbox_id"],
             "total_points": s["total_points"], "points_inside_bbox": s["points_inside_bbox"],
             "points_outside_bbox": s["points_outside_bbox"], "inside_percentage": round(s["inside_percentage"], 2),
             "outside_percentage": round(s["outside_percentage"], 2), "is_matched": s["matched_bbox_id"] >= 0,
             "timestamp": ts} for s in car_statistics]


def _csv_cell(v):
    """one value as pandas' to_csv writes it: bool -> True / False, integer -> digits, float -> shortest repr"""
    if isinstance(v, (bool, np.bool_)):
        return "True" if v else "False"
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    return v


def append_to_master_csv(car_statistics, frame_number, master_csv_path="results/master_car_statistics.csv", timestamp=None):
    if not car_statistics:
        return
    import csv
    d = os.path.dirname(master_csv_path)
    if d:
        os.makedirs(d, exist_ok=True)
    # The bytes pandas' DataFrame(rows).to_csv(index=False) writes (cvs_erosion.py:257-265) -- integers as they are, floats by their
    # shortest repr, booleans as True / False, minimal quoting, "\n" -- without building a DataFrame per frame: in a frame loop the
    # DataFrame cost more than the frame's kernels (tests/test_pipeline_host.py compares the two writers byte for byte).
    rows = csv_rows(car_statistics, frame_number, timestamp)
    new_file = not os.path.exists(master_csv_path)
    with open(master_csv_path, "a", newline="") as fh:
        w = csv.writer(fh, lineterminator="\n")
        if new_file:
            w.writerow(CSV_COLUMNS)
        for r in rows:
            w.writerow([_csv_cell(r[c]) for c in CSV_COLUMNS])
    if new_file:
        print(f"Created new master CSV: {master_csv_path}")
    else:
        print(f"Appended {len(rows)} rows to master CSV: {master_csv_path}")


def analyze_master_csv(master_csv_path="results/master_car_statistics.csv"):
    if not os.path.exists(master_csv_path):
        print(f"Master CSV file not found: {master_csv_path}")
        return
    import pandas as pd
    df = pd.read_csv(master_csv_path)
    print(f"\n{'=' * 60}")
    print(f"{'OVERALL ANALYSIS':^60}")
    print(f"{'=' * 60}")
    print(f"Total frames processed: {df['frame'].nunique()}")
    print(f"Total car detections: {len(df)}")
    print(f"Successfully matched cars: {df['is_matched'].sum()}")
    print(f"Unmatched cars: {(~df['is_matched']).sum()}")
    print(f"Average matching rate: {df['is_matched'].mean() * 100:.1f}%")
    m = df[df["is_matched"] == True]  # noqa: E712  (same comparison as the reference)
    if len(m) > 0:
        print(f"\nMatched Cars Statistics:")
        print(f"Average points per car: {m['total_points'].mean():.1f}")
        print(f"Average inside percentage: {m['inside_percentage'].mean():.1f}%")
        print(f"Min inside percentage: {m['inside_percentage'].min():.1f}%")
        print(f"Max inside percentage: {m['inside_percentage'].max():.1f}%")
    return df


# ---------------------------------------------------------------------------------------
# the fused per-frame path: one batched launch set for many frames
# ---------------------------------------------------------------------------------------
def default_colors(n):
    """(int(i*60)%255, int(i*120)%255, int(i*180)%255), V3:100."""
    return [(int(i * 60) % 255, int(i * 120) % 255, int(i * 180) % 255) for i in range(n)]


class _LiveScanPoints:
    """The pinned points of a reader's Scan for the lazy gathers: indexable like the array while the scan is the reader's current one,
    an LpfError afterwards (its buffers hold another scan by then)."""
    __slots__ = ("scan",)

    def __init__(self, scan):
        self.scan = scan

    def __getitem__(self, key):
        self.scan._check_live()
        return self.scan.points[key]


class FrameResult(dict):
    """run_frames' dict of one frame.  The integers the kernels produced (valid_indices, count_mb, car_statistics, n_valid) are there
    at once; the arrays of the reference's types that are GATHERS or CASTS of them -- ``points_valid`` (V3:592), ``car_point_sets``
    (V3:228), ``u_valid`` / ``v_valid`` as int64 (V3:590-591), ``bg_assigned`` (V4:290-298) -- are made when they are first read (and
    kept): a caller that writes the CSV never pays for 25 000-row fancy-index gathers it does not look at.  Every way of looking at a
    dict sees the same keys and values as before."""
    __slots__ = ("_lazy",)

    def __init__(self, eager, lazy):
        super().__init__(eager)
        self._lazy = dict(lazy)                              # key -> zero-argument callable

    def __missing__(self, key):
        make = self._lazy.pop(key)                           # KeyError for a key that is neither
        val = make()
        self[key] = val
        return val

    def _all(self):
        for k in list(self._lazy):
            self[k]                                          # noqa: B018  (materialises)
        return self

    def get(self, key, default=None):
        return self[key] if (key in self._lazy or dict.__contains__(self, key)) else default

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._lazy

    def __iter__(self):
        return dict.__iter__(self._all())

    def __len__(self):
        return dict.__len__(self) + len(self._lazy)

    def keys(self):
        return dict.keys(self._all())

    def values(self):
        return dict.values(self._all())

    def items(self):
        return dict.items(self._all())

    def copy(self):
        return dict(self._all())

    def __eq__(self, other):
        return dict.__eq__(self._all(), other)

    __hash__ = None

    def __repr__(self):
        return dict.__repr__(self._all())

    def __reduce__(self):                                    # pickles (and deep-copies) as the plain dict it stands for
        return (dict, (dict(self._all()),))


class _DevicePoints:
    """points[idx, :3] of a float32 [N,4] torch tensor on the GPU, as a NumPy array: the gather runs where the points are"""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, key):
        idx, cols = key
        import torch
        i = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.t.device)
        return self.t[i][:, cols].cpu().numpy()


class FrameInputs:
    """What one frame hands to the hot path: velodyne points, detection masks and the
    visible boxes already in velodyne coordinates."""

    def __init__(self, frame, points, masks=None, bboxes_3d=None, colors=None, boxes_2d=None):
        self.frame = frame
        # (a Scan of the read-ahead reader or a float32 [N,4] torch tensor already on the GPU is taken as it is: no host copy)
        self.points = points if (isinstance(points, Scan) or _is_device_tensor(points)) else _f32_points(points).reshape(-1, 4)
        self.masks = masks
        self.bboxes_3d = bboxes_3d if bboxes_3d is not None else []
        n = 0 if masks is None else len(masks)
        self.colors = colors if colors is not None else default_colors(n)
        self.boxes_2d = boxes_2d


def _host_masks_to_device_batch(stacks, M, H, W, ctx):
    """[F,M,H,W] torch tensor on the context's GPU holding the frames' host masks (float32 if any frame's are, else uint8; frames
    with fewer detections padded with empty masks), or None when torch / its GPU support is not there."""
    try:
        import torch
        if not torch.cuda.is_available():
            return None
    except Exception:
        return None
    flt = any(s.dtype == np.float32 for s in stacks if s.shape[0])
    dev = torch.device("cuda", ctx.device)
    ragged = any(s.shape[0] != M for s in stacks)
    t = (torch.zeros if ragged else torch.empty)((len(stacks), M, H, W), dtype=torch.float32 if flt else torch.uint8, device=dev)
    for i, s in enumerate(stacks):
        if s.shape[0]:
            t[i, :s.shape[0]].copy_(torch.from_numpy(s if s.dtype == (np.float32 if flt else np.uint8) else s.astype(np.float32 if flt else np.uint8)))
    ctx.wait_for_stream(torch.cuda.current_stream(dev).cuda_stream)    # the copies were queued on torch's stream
    return t


def _frame_mask_stacks(frames, camera, ctx, erode_iters, v3_pipeline, erosion_kernel_size=3):
    """(per-frame mask stacks at the camera's size, erode_iters, v3_pipeline still owed to the pass) of a batch: the one place that
    decides how masks of another size than the camera's are treated.  They go through cv2.resize as V3:222 does it, on the GPU; with
    the V3 erosion block in force they are eroded at their own size first, as V3:82-97 does before V3:222 (_mask_stack's chain), and
    then so are the batch's other frames, by the same chain -- a batch is eroded either all in the pass or all here.  Which frames
    took the chain is what _mask_stack reports, whatever form their masks came in."""
    def stack(f, force_chain=False):
        return _mask_stack(f.masks if f.masks is not None else [], camera, resize_ctx=ctx, erode_iters=erode_iters,
                           v3_pipeline=v3_pipeline, force_chain=force_chain, erosion_kernel_size=erosion_kernel_size)
    done = [stack(f) for f in frames]
    if not any(eroded for _, eroded in done):
        return [s for s, _ in done], erode_iters, v3_pipeline
    return [s if eroded else stack(f, force_chain=True)[0] for f, (s, eroded) in zip(frames, done)], 0, False


def _mask_batch(stacks, M, H, W, ctx):
    """The frames' mask stacks as ONE [F,M,H,W] batch for a pass (frames with fewer detections padded with empty masks)."""
    on_gpu = [_is_device_tensor(s) for s in stacks]
    if any(on_gpu):                                                      # YOLO's masks still on the GPU: no host round trip
        import torch
        if not all(on_gpu) or any(s.shape[0] != M or s.dtype != stacks[0].dtype for s in stacks):
            raise NotImplementedError("device masks: every frame of a batch needs the same detection count and dtype")
        batch = stacks[0][None] if len(stacks) == 1 else torch.stack(stacks)
        ctx.wait_for_stream(torch.cuda.current_stream(batch.device).cuda_stream)    # the masks were produced on torch's stream
        return batch
    if len(stacks) > 1 and (batch := _host_masks_to_device_batch(stacks, M, H, W, ctx)) is not None:
        # several frames of host masks: each frame's masks go to their place in ONE device tensor -- no np.stack of the batch on the
        # host first (32 frames of five float masks are 340 MB: the copy cost more than everything else in the call)
        return batch
    dt = np.float32 if any(s.dtype == np.float32 for s in stacks if s.shape[0]) else np.uint8
    if all(s.shape[0] == M and s.dtype == dt for s in stacks):
        return stacks[0][None] if len(stacks) == 1 else np.stack(stacks)     # the usual case: no padding, no extra copy
    batch = np.zeros((len(stacks), M, H, W), dt)                         # ragged detection counts: pad with empty masks
    for i, s in enumerate(stacks):
        if s.shape[0]:
            batch[i, :s.shape[0]] = s
    return batch


# What run_frames' collector needs of a compact form of masks beyond its class (_native.MASK_FORMS): the frame a batch gives a frame
# without masks, and its two refusals
def _empty_rle(first, H, W, frame):
    return RleMasks(np.zeros((0, 2), np.int32), np.zeros(1, np.int64), (0, H, W))


def _empty_ids(first, H, W, frame):
    if first.on_device:                                     # (the maps of a GPU batch are the frames of one tensor)
        raise ValueError("frame %s: no masks in a batch of GPU ID maps: give it IdMasks(t[f], []) over its frame of the batch's "
                         "tensor" % (frame,))
    return IdMasks(np.zeros((H, W), first.id_dtype), [])


_FRAME_FORMS = {
    "rle": (RleMasks, _empty_rle, "frame %s: RleMasks of %d x %d, the camera is %d x %d (runs are not resized: decode with .to_dense())",
            "frame %s: dense masks in a batch of RleMasks frames: one form per batch (.to_dense() or RleMasks.from_dense)"),
    "ids": (IdMasks, _empty_ids, "frame %s: an ID map of %d x %d, the camera is %d x %d (maps are not resized: use .to_dense())",
            "frame %s: another form of masks in a batch of IdMasks frames: one form per batch (.to_dense())")}


def _compact_frame_masks(frames, camera, forms, size=None):
    """``(form, each frame's masks in it)`` when the batch's masks come in one of the compact ``forms`` ("rle": RleMasks, "ids":
    IdMasks; tried in that order), None when no frame's do.  A frame without masks -- None, an empty list -- gets an empty instance:
    no runs, or no ``sel`` over a zero host map of the batch's ID dtype.  ValueError, before anything reaches the library: a batch
    that mixes the form with another, masks of another size than the camera's (neither runs nor maps are resized) -- or than ``size`` =
    (H, W), for a call that reads masks at a size of their own -- and a frame without masks among GPU ID maps."""
    for form in forms:
        cls, empty, wrong_size, mixed = _FRAME_FORMS[form]
        first = next((f.masks for f in frames if isinstance(f.masks, cls)), None)
        if first is None:
            continue
        H, W = size or (camera.height, camera.width)
        out = []
        for f in frames:
            if isinstance(f.masks, cls):
                if tuple(f.masks.shape[1:]) != (H, W):
                    raise ValueError(wrong_size % (f.frame, f.masks.shape[2], f.masks.shape[1], W, H))
                out.append(f.masks)
            elif f.masks is None or len(f.masks) == 0:
                out.append(empty(first, H, W, f.frame))
            else:
                raise ValueError(mixed % (f.frame,))
        return form, out
    return None


def _run_frames_compact(frames, form, masks, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, device, ctx,
                        gather_scans, erosion_kernel_size):
    """run_frames for frames whose masks are in a compact form -- ``masks``: each frame's RleMasks ("rle") or IdMasks ("ids") -- with
    the camera and the erosion element set: up to 32 masks in one narrow pass behind set_masks_rle / set_masks_ids, 33 to 256 in ONE
    wide pass (run_wide takes either form as it is), more in groups of 256, by slices (those of an IdMasks share the map).  The runs
    or the map go to the GPU -- a GPU map is read where it is -- not the masks.  On 0/1 masks V3's cast chain is the erosion alone, so
    v3_pipeline needs nothing beyond erode_iters."""
    counts = [m.shape[0] for m in masks]
    if max(counts) > LPF_MAX_MASKS_WIDE:
        return _run_frames_in_mask_groups(frames, masks, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, False,
                                          device, ctx, group=LPF_MAX_MASKS_WIDE, erosion_kernel_size=erosion_kernel_size)
    corners, positions = zip(*(_corners_velo(f.bboxes_3d) for f in frames))
    pts = [f.points for f in frames]
    if max(counts) > LPF_MAX_MASKS:
        ctx.set_boxes(list(corners), oriented=use_oriented)
        res = ctx.run_wide(pts, masks, erode_iters=erode_iters, want_uv=False, want_valid_uv=True)
    else:
        getattr(ctx, "set_masks_" + form)(masks, erode_iters=erode_iters)       # set_masks_rle, set_masks_ids
        ctx.set_boxes(list(corners), oriented=use_oriented)
        res = ctx.run_batch(pts, want_uv=False, want_label=False, want_valid_uv=True, pinned=True)
    return [_frame_result(f, r, m, pos, min_points, gather_scans) for f, r, m, pos in zip(frames, res, counts, positions)]


def run_frames(frames, TrVeloToRect, camera, depth_max=50.0, min_points=10, use_oriented=True,
               erode_iters=0, v3_pipeline=False, device=0, ctx=None, gather_scans=True, erosion_kernel_size=3):
    """Projection + clip + mask lookup + box counting + best-box scan for a list of
    FrameInputs in ONE batched call (frames are independent units).  Returns one dict per
    frame: valid_indices, u_valid, v_valid, points_valid, car_point_sets, bg_assigned,
    count_mb, car_statistics (cvs_erosion key set) -- the integers are the kernels' output,
    the dicts are assembled here.  Frames whose points are a read-ahead reader's ``Scan`` have their gathers (``points_valid``,
    ``car_point_sets``) made before the call returns, because the reader recycles the scan's buffers when it moves on;
    ``gather_scans=False`` leaves them lazy like everyone else's -- reading them after the reader has moved on raises.
    ``erosion_kernel_size``: the reference's knob of that name (V3:55, cvs_erosion.py:77) -- ``erode_iters`` iterations erode with the
    k x k MORPH_ELLIPSE element (odd, 1 .. 15; 3 is the cross).  It is set on the context by every call, the default included.
    Frames whose ``masks`` are in a compact form -- ``rle.RleMasks``, or ``idmap.IdMasks`` (instance-ID maps of one ID dtype, all in
    host memory or all the frames of one GPU tensor); at the camera's size; every frame of the batch, a frame without masks aside --
    take set_masks_rle / set_masks_ids, or with 33 to 256 masks ONE run_wide pass: the labels are built from the runs or the map on
    the GPU, nothing dense crosses to the device or exists anywhere; more than 256 masks run in groups of 256.  One form per batch."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if not frames:
        return []
    compact = _compact_frame_masks(frames, camera, ("rle", "ids"))
    ctx = ctx or get_context(device)
    ctx.set_erosion_element(erosion_kernel_size)
    H, W = camera.height, camera.width
    ctx.set_camera(TrVeloToRect, camera.K, W, H, 0.0, float(depth_max))
    if compact is not None:
        return _run_frames_compact(frames, *compact, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, device, ctx,
                                   gather_scans, erosion_kernel_size)
    stacks, erode_iters, v3_pipeline = _frame_mask_stacks(frames, camera, ctx, erode_iters, v3_pipeline, erosion_kernel_size)
    counts = [s.shape[0] for s in stacks]
    M = max(counts)
    if M > LPF_MAX_MASKS_WIDE:
        # The reference loops over every mask (V3:220), with no bound: beyond what one wide pass takes, the frames run once per group
        # of 256 masks and the per-detection results are put together
        return _run_frames_in_mask_groups(frames, stacks, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters,
                                          v3_pipeline, device, ctx, group=LPF_MAX_MASKS_WIDE, erosion_kernel_size=erosion_kernel_size)
    res, positions = _frames_pass(frames, stacks, M, camera, use_oriented, erode_iters, v3_pipeline, ctx)
    return [_frame_result(f, r, m, pos, min_points, gather_scans) for f, r, m, pos in zip(frames, res, counts, positions)]


def _frames_pass(frames, stacks, M, camera, use_oriented, erode_iters, v3_pipeline, ctx, staged=None):
    """ONE native pass over frames of up to 256 masks each (``stacks`` at the camera's size, the camera set): (the pass's dict per
    frame, each frame's box positions).  It leaves the frames' boxes in force.  staged: the frames' points as ctx.stage_points put them."""
    batch = _mask_batch(stacks, M, camera.height, camera.width, ctx)
    corners, positions = zip(*(_corners_velo(f.bboxes_3d) for f in frames))
    pts = [f.points for f in frames]
    # only the valid points' pixels and labels are used below: fetch those (a quarter of the dense arrays on real frames)
    if M <= LPF_MAX_MASKS:
        ctx.set_masks(batch, erode_iters=erode_iters, v3_pipeline=v3_pipeline, lend=True)   # (the run follows in this call: GPU masks can be lent)
        ctx.set_boxes(list(corners), oriented=use_oriented)
        # (results arrive in page-locked buffers the context reuses: _frame_result copies out what is handed to the caller)
        res = ctx.run_batch(pts, want_uv=False, want_label=False, want_valid_uv=True, pinned=True, staged=staged)
    else:
        # A launch of the narrow path labels a point with one bit per mask in a 32-bit word; more detections than that take the wide
        # pass (lpf_run_wide: ceil(M / 32) label words per point), which projects and reads every point once
        ctx.set_boxes(list(corners), oriented=use_oriented)
        res = ctx.run_wide(pts, batch, erode_iters=erode_iters, v3_pipeline=v3_pipeline, want_uv=False, want_valid_uv=True, staged=staged)
    return res, positions


def _frame_result(f, r, m, pos, min_points, gather_scans):
    """The FrameResult of frame ``f`` (``m`` detections, boxes at ``pos`` of its list) from the pass's dict ``r``: run_batch's, whose
    label_valid holds one word per valid point, or run_wide's, whose label_valid_words hold ceil(M / 32)."""
    # (the result arrays may live in page-locked buffers the context reuses: what outlives this call is copied out of them here -- the
    #  compact lists, a few hundred KB -- and the gathers / casts of the reference's types are made from those copies when read)
    vi = r["valid_idx"].copy()
    uvv = r["uv_valid"].copy()                                           # int32 [n_valid, 2]: one contiguous copy
    labv = (r["label_valid"] if "label_valid" in r else r["label_valid_words"]).copy()
    lists = [l.copy() for l in r["inst_lists"][:m]]
    is_scan = isinstance(f.points, Scan)
    host_pts = _LiveScanPoints(f.points) if is_scan else f.points        # Scan: pinned copy of the file, while the reader has not moved on
    if _is_device_tensor(host_pts):                                      # points that live on the GPU: the gathers run there when asked for
        host_pts = _DevicePoints(host_pts)
    stats = []
    if f.bboxes_3d and m:
        stats = stats_from_counts(r["inst_count"][:m], r["count_mb"][:m], f.colors, min_points, pos)
        for d in stats:
            d.pop("_best_col"), d.pop("_best_count")
    lazy = dict(u_valid=lambda uvv=uvv: uvv[:, 0].astype(np.int64), v_valid=lambda uvv=uvv: uvv[:, 1].astype(np.int64),
                points_valid=lambda p=host_pts, vi=vi: p[vi, :3],
                car_point_sets=lambda p=host_pts, ls=lists: [p[l, :3] if len(l) else np.array([]).reshape(0, 3) for l in ls],
                bg_assigned=lambda labv=labv: labv != 0 if labv.ndim == 1 else (labv != 0).any(axis=1))
    fr = FrameResult(dict(frame=f.frame, valid_indices=vi, count_mb=r["count_mb"][:m].copy(), car_statistics=stats, n_valid=r["n_valid"]), lazy)
    if is_scan and gather_scans:
        fr._all()                                            # (a Scan's pinned points are recycled when the reader moves on: gather now)
    return fr


def _run_frames_in_mask_groups(frames, stacks, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, v3_pipeline,
                               device, ctx, group=LPF_MAX_MASKS, erosion_kernel_size=3):
    """run_frames for frames with more masks than one pass takes: one pass per group of ``group`` masks, results merged.  (With the
    default 32 every pass is the narrow path: the yardstick of the wide pass.)"""
    M = max(s.shape[0] for s in stacks)
    merged = None
    for g0 in range(0, M, group):
        part = [FrameInputs(f.frame, f.points, s[g0:g0 + group], f.bboxes_3d, f.colors[g0:g0 + group], f.boxes_2d)
                for f, s in zip(frames, stacks)]
        res = run_frames(part, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, v3_pipeline, device, ctx,
                         erosion_kernel_size=erosion_kernel_size)
        if merged is None:
            merged = res
            continue
        for acc, r in zip(merged, res):
            acc["car_point_sets"] += r["car_point_sets"]
            acc["bg_assigned"] = acc["bg_assigned"] | r["bg_assigned"]
            acc["count_mb"] = np.concatenate([acc["count_mb"], r["count_mb"]], axis=0)
            for d in r["car_statistics"]:
                d["car_id"] += g0                            # car ids count the detections of the whole frame (V3:330)
            acc["car_statistics"] += r["car_statistics"]
    return merged


# ---------------------------------------------------------------------------------------
# V3's key set for a batch: corners_velo, inside_mask, car_points (V3:386-398, V3:413-425) and the cloud of V3:606-621
# ---------------------------------------------------------------------------------------
def inside_list_arrays(res, M):
    """The instance lists of a pass (run_batch's / run_wide's dicts, M masks wide) as lpf_inside_masks takes them: inst_idx int64
    [F, inst_cap], inst_off int64 [F, M + 1], best_box int32 [F, M], best_cnt int64 [F, M]."""
    F = len(res)
    inst_off = np.zeros((F, M + 1), np.int64)
    best_box, best_cnt = np.full((F, M), -1, np.int32), np.zeros((F, M), np.int64)
    for f, r in enumerate(res):
        inst_off[f, 1:] = np.cumsum(r["inst_count"][:M])
        best_box[f], best_cnt[f] = r["best_box"][:M], r["best_cnt"][:M]
    inst_idx = np.zeros((F, max(int(inst_off[:, M].max()) if F else 0, 1)), np.int64)
    for f, r in enumerate(res):
        if inst_off[f, M]:
            inst_idx[f, :inst_off[f, M]] = np.concatenate(r["inst_lists"][:M])
    return inst_idx, inst_off, best_box, best_cnt


def merge_inside_parts(a, b):
    """The ``inside_parts`` of one frame over two groups of masks, group ``a``'s cars first (frames with more masks than one pass takes)."""
    return dict(part_idx=np.concatenate([a["part_idx"], b["part_idx"]]), part_xyz=np.concatenate([a["part_xyz"], b["part_xyz"]]),
                off=np.concatenate([a["off"], b["off"][1:] + a["off"][-1]]), n_inside=np.concatenate([a["n_inside"], b["n_inside"]]),
                matched=np.concatenate([a["matched"], b["matched"]]))


def car_statistics_v3_frames(frames, TrVeloToRect, camera, depth_max=50.0, min_points=10, use_oriented=True, erode_iters=0,
                             v3_pipeline=False, device=0, ctx=None, erosion_kernel_size=3):
    """run_frames whose ``car_statistics`` carry V3's key set (V3:386-398, V3:413-425): next to the counts ``corners_velo`` (f64 [8,3]
    or None), ``inside_mask`` (bool [k], None for a car without a box) and ``car_points`` -- what calculate_car_point_statistics
    (style 'v3') returns for each frame, from run_frames' pass plus ONE lpf_inside_masks call for the whole batch: each list entry is
    tested against its car's best box on the GPU, instead of every car point against every box of the frame in a blocking call per
    frame.  The points are staged once for both.  Each frame's dict also has ``inside_parts`` -- part_idx int64 [sum k], part_xyz
    float32 [sum k, 3] (per car: the points inside its box first, then the others), off int64 [m + 1], n_inside int64 [m], matched
    bool [m] -- which inside_outside_cloud_frames turns into V3's cloud.  Frames with more than 256 masks run once per group of 256.
    ``erosion_kernel_size``: as in run_frames."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if not frames:
        return []
    ctx = ctx or get_context(device)
    ctx.set_erosion_element(erosion_kernel_size)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    stacks, erode_iters, v3_pipeline = _frame_mask_stacks(frames, camera, ctx, erode_iters, v3_pipeline, erosion_kernel_size)
    counts = [s.shape[0] for s in stacks]
    M = max(counts)
    if M > LPF_MAX_MASKS_WIDE:
        merged = None
        for g0 in range(0, M, LPF_MAX_MASKS_WIDE):
            part = [FrameInputs(f.frame, f.points, s[g0:g0 + LPF_MAX_MASKS_WIDE], f.bboxes_3d, f.colors[g0:g0 + LPF_MAX_MASKS_WIDE], f.boxes_2d)
                    for f, s in zip(frames, stacks)]
            res = car_statistics_v3_frames(part, TrVeloToRect, camera, depth_max, min_points, use_oriented, erode_iters, v3_pipeline, device, ctx,
                                           erosion_kernel_size)
            if merged is None:
                merged = res
                continue
            for acc, r in zip(merged, res):
                acc["car_point_sets"] += r["car_point_sets"]
                acc["bg_assigned"] = acc["bg_assigned"] | r["bg_assigned"]
                acc["count_mb"] = np.concatenate([acc["count_mb"], r["count_mb"]], axis=0)
                for d in r["car_statistics"]:
                    d["car_id"] += g0                        # car ids count the detections of the whole frame (V3:330)
                acc["car_statistics"] += r["car_statistics"]
                acc["inside_parts"] = merge_inside_parts(acc["inside_parts"], r["inside_parts"])
        return merged
    staged = ctx.stage_points([f.points for f in frames])    # one copy of the batch's points for the pass and the split
    res, positions = _frames_pass(frames, stacks, M, camera, use_oriented, erode_iters, v3_pipeline, ctx, staged=staged)
    inst_idx, inst_off, best_box, best_cnt = inside_list_arrays(res, M)
    # (_frame_result copies what it keeps out of the pass's page-locked buffers; the list arrays above are copies already)
    out = [_frame_result(f, r, m, pos, min_points, True) for f, r, m, pos in zip(frames, res, counts, positions)]
    split = ctx.inside_masks(None, inst_idx, inst_off, best_box, best_cnt, min_points=min_points, staged=staged)
    for i, (f, fr, m) in enumerate(zip(frames, out, counts)):
        off = inst_off[i, :m + 1].copy()
        tot = int(off[m])
        fr["inside_parts"] = dict(part_idx=split["part_idx"][i, :tot].copy(), part_xyz=split["part_xyz"][i, :tot].copy(), off=off,
                                  n_inside=split["n_inside"][i, :m].copy(), matched=split["matched"][i, :m] != 0)
        if not fr["car_statistics"]:
            continue
        sets = fr["car_point_sets"]
        for d in fr["car_statistics"]:
            car = d["car_id"]
            if d["matched_bbox_id"] >= 0:
                d["corners_velo"] = np.array(f.bboxes_3d[d["matched_bbox_id"]]["corners_velo"])
                d["inside_mask"] = split["inside"][i, off[car]:off[car + 1]] != 0
            else:
                d["corners_velo"] = None
                d["inside_mask"] = None
            d["car_points"] = sets[car]
    return out


def inside_outside_cloud_frames(results, background=(0.5, 0.5, 0.5)):
    """The geometry list of V3:606-621 as arrays, for each dict of car_statistics_v3_frames: ``points`` float32 [n,3], ``colors``
    float64 [n,3] and ``parts`` int32 [n,2] = (car id, code) with code 0 an unmatched car's point, 1 inside its car's box, 2 outside
    it, 3 background (car id -1).  The order is the reference's: per statistics dict an unmatched car's points (V3:481-487), a matched
    car's inside points and then its outside points (V3:493-507), and the points of no car last (V3:618-621:
    points_valid[~bg_assigned]).  A car's colour is color[::-1] / 255.0 for all of its points -- the reference computes the same
    colour for the outside points (V3:504); ``parts`` is what lets a caller tint them apart.  The cars' points are slices of the
    GPU's inside-first partition (``inside_parts``), not boolean gathers per car."""
    clouds = []
    bg_color = np.asarray(background, np.float64).reshape(1, 3)
    for r in results:
        ip = r["inside_parts"]
        off, xyz = ip["off"], ip["part_xyz"]
        pts, cols, parts = [], [], []
        for d in r["car_statistics"]:
            car = d["car_id"]
            a, b = int(off[car]), int(off[car + 1])
            col = d["color"]
            pts.append(xyz[a:b])
            cols.append(np.tile(np.array([col[2], col[1], col[0]]) / 255.0, (b - a, 1)))
            code = np.zeros((b - a, 2), np.int32)
            code[:, 0] = car
            if d["matched_bbox_id"] >= 0:
                code[:, 1] = 2
                code[:int(ip["n_inside"][car]), 1] = 1
            parts.append(code)
        rest = np.asarray(r["points_valid"])[~np.asarray(r["bg_assigned"])]
        pts.append(rest.astype(np.float32, copy=False).reshape(-1, 3))
        cols.append(np.tile(bg_color, (len(rest), 1)))
        parts.append(np.tile(np.array([[-1, 3]], np.int32), (len(rest), 1)))
        clouds.append(dict(frame=r["frame"], points=np.concatenate(pts).astype(np.float32, copy=False),
                           colors=np.concatenate(cols).astype(np.float64, copy=False).reshape(-1, 3), parts=np.concatenate(parts)))
    return clouds


# ---------------------------------------------------------------------------------------
# point-level recall: how many of the LiDAR points in a car's annotated box does its mask still cover?
# ---------------------------------------------------------------------------------------
RECALL_COLUMNS = CSV_COLUMNS + ("bbox_lidar_points", "recall_percentage")


def point_recall_frames(frames, TrVeloToRect, camera, depth_max=50.0, min_points=10, use_oriented=True, erode_iters=0,
                        v3_pipeline=False, device=0, erosion_kernel_size=3, ctx=None):
    """run_frames plus the recall side of its statistics, from run_frames' pass and ONE lpf_box_points call for the whole batch (the
    points are staged once for both): the box test on ALL valid points of a frame, not only on the masked ones.  Each frame's dict
    is run_frames' plus
      ``box_points`` / ``box_labelled``  int32, one entry per box of the frame's list, at the positions ``matched_bbox_id`` refers
                           to: the valid points inside the box, and those of them some mask covers (0 for a list entry without corners);
      ``first_box``        int32, parallel to ``valid_indices``: the first box of the list that holds the point, -1 if none;
      ``point_confusion``  {"tp", "fp", "fn", "tn"} of "car vs. not car" per valid point: tp labelled and in a box, fp labelled and in
                           no box, fn unlabelled and in a box, tn neither;
    and in every ``car_statistics`` dict ``bbox_lidar_points`` (box_points of the matched box, 0 for an unmatched car) and
    ``recall_percentage`` (points_inside_bbox / bbox_lidar_points * 100, 0.0 for an unmatched car).  Frames with more than 256 masks
    run once per group of 256; a point counts as labelled when any group labels it.  ``erosion_kernel_size``: as in run_frames."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if not frames:
        return []
    ctx = ctx or get_context(device)
    ctx.set_erosion_element(erosion_kernel_size)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    stacks, erode_iters, v3_pipeline = _frame_mask_stacks(frames, camera, ctx, erode_iters, v3_pipeline, erosion_kernel_size)
    M = max(s.shape[0] for s in stacks)
    staged = ctx.stage_points([f.points for f in frames])    # one copy of the batch's points for the passes and the box test
    off = staged[0]
    valid, n_valid, labels, out = np.zeros(int(off[-1]), np.int64), np.zeros(len(frames), np.int64), None, None
    G = LPF_MAX_MASKS_WIDE
    for g0 in range(0, max(M, 1), G):
        part = frames if M <= G else [FrameInputs(f.frame, f.points, None, f.bboxes_3d, f.colors[g0:g0 + G], f.boxes_2d) for f in frames]
        pstacks = stacks if M <= G else [s[g0:g0 + G] for s in stacks]
        counts = [s.shape[0] for s in pstacks]
        res, positions = _frames_pass(part, pstacks, max(counts), camera, use_oriented, erode_iters, v3_pipeline, ctx, staged=staged)
        # the compact lists of the pass as the box test takes them (copies: the pass's arrays may live in buffers the context reuses)
        for i, r in enumerate(res):
            a, n = int(off[i]), int(r["n_valid"])
            lab = r["label_valid"] if "label_valid" in r else r["label_valid_words"]
            if M > G:                                        # several groups: one word per point, non-zero where any group labels it
                lab = (lab != 0) if lab.ndim == 1 else (lab != 0).any(axis=1)
            if labels is None:
                labels = np.zeros((len(valid),) + tuple(np.shape(lab)[1:]), np.uint32)
            if g0 == 0:
                valid[a:a + n], n_valid[i] = r["valid_idx"], n
                labels[a:a + n] = lab
            else:
                labels[a:a + n] |= lab.astype(np.uint32)
        got = [_frame_result(f, r, m, pos, min_points, True) for f, r, m, pos in zip(part, res, counts, positions)]
        if out is None:
            out = got
            continue
        for acc, r in zip(out, got):
            acc["car_point_sets"] += r["car_point_sets"]
            acc["bg_assigned"] = acc["bg_assigned"] | r["bg_assigned"]
            acc["count_mb"] = np.concatenate([acc["count_mb"], r["count_mb"]], axis=0)
            for d in r["car_statistics"]:
                d["car_id"] += g0                            # car ids count the detections of the whole frame (V3:330)
            acc["car_statistics"] += r["car_statistics"]
    bp = ctx.box_points(None, valid, n_valid, labels, staged=staged)
    box_off = ctx.box_off
    for i, (f, fr, pos) in enumerate(zip(frames, out, positions)):
        b0, b1, a, n = int(box_off[i]), int(box_off[i + 1]), int(off[i]), int(n_valid[i])
        pos = np.asarray(pos, np.int64)
        per_box = {}
        for k in ("box_points", "box_labelled"):
            per_box[k] = np.zeros(len(f.bboxes_3d), np.int32)
            per_box[k][pos] = bp[k][b0:b1]
            fr[k] = per_box[k]
        first = bp["first_box"][a:a + n]
        fr["first_box"] = np.where(first >= 0, pos[np.maximum(first, 0)] if len(pos) else -1, -1).astype(np.int32)
        valid_n, boxed, lab, both = (int(x) for x in bp["frame_counts"][i])
        fr["point_confusion"] = {"tp": both, "fp": lab - both, "fn": boxed - both, "tn": valid_n - boxed - lab + both}
        for d in fr["car_statistics"]:
            if d["matched_bbox_id"] >= 0:
                d["bbox_lidar_points"] = int(per_box["box_points"][d["matched_bbox_id"]])
                d["recall_percentage"] = d["points_inside_bbox"] / d["bbox_lidar_points"] * 100
            else:
                d["bbox_lidar_points"], d["recall_percentage"] = 0, 0.0
    return out


def recall_rows(results, timestamp=None):
    """One row per car of point_recall_frames' results: csv_rows' columns plus ``bbox_lidar_points`` and ``recall_percentage``
    (RECALL_COLUMNS; the percentage rounded to two places like the others).  csv_rows and the master CSV's schema stay as they are."""
    rows = []
    for r in results:
        for row, s in zip(csv_rows(r["car_statistics"], r["frame"], timestamp), r["car_statistics"]):
            row["bbox_lidar_points"] = s["bbox_lidar_points"]
            row["recall_percentage"] = round(s["recall_percentage"], 2)
            rows.append(row)
    return rows


def _n_points(points):
    return len(points.points) if isinstance(points, Scan) else int(points.shape[0])


def run_frames_multicam(frames_per_cam, cams, depth_max=50.0, min_points=10, use_oriented=True, erode_iters=0, v3_pipeline=False,
                        device=0, ctx=None, gather_scans=True, erosion_kernel_size=3):
    """run_frames for the same frames seen by up to four cameras, in ONE native pass (LpfContext.run_cams): every scan is staged and
    read once, however many cameras label it.  ``cams[c] = (TrVeloToRect, camera)``; ``frames_per_cam[c]`` is camera c's list of
    FrameInputs -- frame i of every camera carries the same points (the same frame id and point count; anything else raises
    ValueError), its own masks, colors and boxes (the boxes camera c sees).  Returns ``results[c][i]`` equal to
    ``run_frames(frames_per_cam[c], *cams[c], ...)[i]``, car_statistics and the lazy keys included.  A camera with a frame of more than
    32 masks goes through run_frames on its own (the pass takes a 32-bit label word per camera); the results are the same.  (Routing
    such cameras through one LpfContext.run_cams_wide pass measured slower per frame than this)
    A camera's frames may carry ``rle.RleMasks`` (run_frames' rules: every frame of that camera, at its size); it is routed by its mask
    count in the same way, and a camera with dense masks and a camera with RleMasks may share the pass.
    ``erosion_kernel_size``: as in run_frames, for every camera."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    C = len(cams)
    if not 1 <= C <= LPF_MAX_CAMS:
        raise ValueError("run_frames_multicam takes 1 to %d cameras, got %d" % (LPF_MAX_CAMS, C))
    if len(frames_per_cam) != C:
        raise ValueError("frames for %d cameras, %d cameras given" % (len(frames_per_cam), C))
    F = len(frames_per_cam[0])
    for c, fs in enumerate(frames_per_cam):
        if len(fs) != F:
            raise ValueError("camera %d has %d frames, camera 0 has %d" % (c, len(fs), F))
        for i, (f, f0) in enumerate(zip(fs, frames_per_cam[0])):
            if f.frame != f0.frame or _n_points(f.points) != _n_points(f0.points):
                raise ValueError("frame %d of camera %d (frame %r, %d points) is not camera 0's (frame %r, %d points): every camera "
                                 "labels the same scans" % (i, c, f.frame, _n_points(f.points), f0.frame, _n_points(f0.points)))
    if F == 0:
        return [[] for _ in range(C)]
    ctx = ctx or get_context(device)
    ctx.set_erosion_element(erosion_kernel_size)
    results = [None] * C
    passes = []                                           # (camera, stacks, counts, M, erode_iters, v3_pipeline)
    for c, (T, camera) in enumerate(cams):
        compact = _compact_frame_masks(frames_per_cam[c], camera, ("rle",))
        if compact is not None:
            # RleMasks frames: routed by M as dense masks are -- the pass takes the runs as they are, run_frames the wider camera (on
            # 0/1 masks V3's cast chain is the erosion alone, _run_frames_compact)
            rles = compact[1]
            counts = [r.shape[0] for r in rles]
            if max(counts) > LPF_MAX_MASKS:
                results[c] = run_frames(frames_per_cam[c], T, camera, depth_max, min_points, use_oriented, erode_iters, v3_pipeline, device,
                                        ctx, gather_scans, erosion_kernel_size)
            else:
                passes.append((c, rles, counts, max(counts), erode_iters, False))
            continue
        # (masks of another size are resized -- and with the V3 block eroded -- at camera c's size: the context's camera for that)
        ctx.set_camera(T, camera.K, camera.width, camera.height, 0.0, float(depth_max))
        stacks, er, v3 = _frame_mask_stacks(frames_per_cam[c], camera, ctx, erode_iters, v3_pipeline, erosion_kernel_size)
        counts = [s.shape[0] for s in stacks]
        if max(counts) > LPF_MAX_MASKS:
            results[c] = run_frames(frames_per_cam[c], T, camera, depth_max, min_points, use_oriented, erode_iters, v3_pipeline, device,
                                    ctx, gather_scans, erosion_kernel_size)
            continue
        passes.append((c, stacks, counts, max(counts), er, v3))
    if not passes:
        return results
    specs, positions = [], []
    for c, stacks, counts, M, er, v3 in passes:
        T, camera = cams[c]
        corners, pos = zip(*(_corners_velo(f.bboxes_3d) for f in frames_per_cam[c]))
        positions.append(pos)
        specs.append(dict(T_velo_to_rect=T, K=camera.K, width=camera.width, height=camera.height, depth_min=0.0, depth_max=float(depth_max),
                          masks=stacks if isinstance(stacks[0], RleMasks) else _mask_batch(stacks, M, camera.height, camera.width, ctx),
                          binarize="v3" if v3 else "astype",
                          erode_iters=er, boxes=list(corners), oriented=use_oriented))
    pts = [f.points for f in frames_per_cam[passes[0][0]]]
    # (results arrive in page-locked buffers the context reuses, one set per camera: _frame_result copies out what it hands on)
    res = ctx.run_cams(pts, specs, want_uv=False, want_label=False, want_valid_uv=True, pinned=True)
    for (c, stacks, counts, M, er, v3), rc, pos in zip(passes, res, positions):
        results[c] = [_frame_result(f, r, m, p, min_points, gather_scans) for f, r, m, p in zip(frames_per_cam[c], rc, counts, pos)]
    return results


def stream_frames(scan_paths, inputs_for, TrVeloToRect, camera, depth_max=50.0, min_points=10, use_oriented=True,
                  erode_iters=0, v3_pipeline=False, device=0, n_buffers=3, max_points=None, box_paths=None, announce=None, gather=True,
                  erosion_kernel_size=3):
    """The frame loop with read-ahead: scans are read and moved to HBM by the native reader
    (lpf_reader_*) while earlier frames are processed; yields run_frames' dict per frame.
    ``inputs_for(i, path)`` returns ``(frame_id, masks, bboxes_3d, colors)`` or None to skip the
    frame (the reference's ``continue`` rules); it runs while the scan is still being fetched.
    A missing scan prints the reference's message (cvs_erosion.py:326-330) and is skipped.
    With ``box_paths`` (one ``BBoxes_<frame>.json`` per scan) the reader's worker parses the box file beside the scan
    (lpf_reader_submit_frame) and ``inputs_for(i, path, scan)`` is called once the scan is there, ``scan.boxes_state`` /
    ``scan.box_index`` / ``scan.boxes_cam0`` holding the result; the scans and box files of the NEXT frames are being fetched
    meanwhile.  ``announce(i, path)`` runs before the scan is waited for (the reference's "Processing frame" line).
    ``gather=False``: the consumer only reads the statistics (process_frames writes the CSV): ``points_valid`` / ``car_point_sets``
    are not gathered from the scan before the reader recycles it (run_frames' ``gather_scans``).  ``erosion_kernel_size``: as in
    run_frames."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    scan_paths = [os.fspath(p) for p in scan_paths]
    if max_points is None:
        sizes = [os.path.getsize(p) // 16 for p in scan_paths if os.path.isfile(p)]
        max_points = max(sizes + [1])
    ctx = get_context(device)
    with ScanReader(ctx, scan_paths, n_buffers=n_buffers, max_points=max_points, box_paths=box_paths) as reader:
        for i, path in enumerate(scan_paths):
            if announce is not None:
                announce(i, path)
            inputs = inputs_for(i, path) if box_paths is None else None
            try:
                scan = next(reader)
            except RuntimeError as e:
                print(f"Failed to load frame {os.path.basename(path)}: {e}")
                continue
            if box_paths is not None:
                inputs = inputs_for(i, path, scan)
            if inputs is None:
                continue
            frame_id, masks, boxes, colors = inputs
            yield run_frames([FrameInputs(frame_id, scan, masks, boxes, colors)], TrVeloToRect, camera, depth_max,
                             min_points, use_oriented, erode_iters, v3_pipeline, device, ctx, gather_scans=gather,
                             erosion_kernel_size=erosion_kernel_size)[0]


# ---------------------------------------------------------------------------------------
# entry points (frame loops of cvs_erosion.py:298-379 and V3:516-641)
# ---------------------------------------------------------------------------------------
def sequence_setup(kitti360_path, seq=0, cam_id=0):
    """camera, TrVeloToCam, TrVeloToRect and the velodyne reader, composed as V3:520-535."""
    sequence = "2013_05_28_drive_%04d_sync" % seq
    camera = kitti360.CameraPerspective(kitti360_path, sequence, cam_id)
    velo_to_cam, velo_to_rect = kitti360.velo_to_rect_transforms(kitti360_path, camera, cam_id)
    velo = kitti360.Kitti360Viewer3DRaw(seq=seq, root_dir=kitti360_path)
    return sequence, camera, velo_to_cam, velo_to_rect, velo


def _boxes_of_file(json_path, camera, velo_to_cam, keep_all=False, parsed=None):
    """load_bounding_boxes (V3:31-38) + prepare_boxes for callers that keep the boxes to themselves; None = the reference's
    ``if not bboxes_3d_raw: continue`` (cvs_erosion.py:334-335: no file -- its message is printed -- or an empty list).  The file is
    parsed by the library (``parsed`` = the read-ahead reader's result for it, else lpf_parse_boxes_json now); a file that is not the
    plain schema goes through json.load as before."""
    state, index, corners = parsed if parsed is not None else _native.parse_boxes_file(json_path)
    if state == _native.BOXES_PARSED:
        return prepare_boxes_from_arrays(index, corners, camera, velo_to_cam, keep_all=keep_all) if len(index) else None
    raw = kitti360.load_bounding_boxes(json_path)           # absent: prints the reference's message, []; other schema: json.load
    if not raw:
        return None
    return prepare_boxes(raw, camera, velo_to_cam, keep_all=keep_all, as_arrays=True)


def collect_frame_inputs(kitti360_path, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames=None,
                         keep_all_boxes=False, boxes_as_arrays=False):
    """iter_frame_inputs as a list (every frame's scan and masks in memory at once: for a handful of frames)."""
    return list(iter_frame_inputs(kitti360_path, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames,
                                  keep_all_boxes, boxes_as_arrays))


def _batches(items, n):
    """Lists of up to n consecutive items of an iterable, made as they are asked for."""
    batch = []
    for it in items:
        batch.append(it)
        if len(batch) >= n:
            yield batch
            batch = []
    if batch:
        yield batch


def iter_frame_inputs(kitti360_path, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames=None,
                      keep_all_boxes=False, boxes_as_arrays=False):
    """The reference's per-frame loading + skip rules (cvs_erosion.py:320-369), one FrameInputs at a time: a frame is
    dropped when its scan, its box file, its image or its detections are missing.  (A generator: a frame loop over a whole drive
    holds one batch of scans and masks, not the drive.)"""
    sequence = "2013_05_28_drive_%04d_sync" % seq
    bbox_dir = os.path.join(kitti360_path, "bboxes_3D_cam0")
    todo = velo.available_frames() if frames is None else list(frames)
    print(f"Found {len(todo)} frames to process")
    for frame in todo:
        print(f"\nProcessing frame {frame}...")
        try:
            points = velo.loadVelodyneData(frame)
        except Exception as e:  # same breadth as the reference
            print(f"Failed to load frame {frame}: {e}")
            continue
        if boxes_as_arrays:                                 # (the caller keeps the boxes to itself: the library parses the file)
            boxes = _boxes_of_file(os.path.join(bbox_dir, f"BBoxes_{frame}.json"), camera, velo_to_cam, keep_all_boxes)
            if boxes is None:
                continue
        else:
            raw = kitti360.load_bounding_boxes(os.path.join(bbox_dir, f"BBoxes_{frame}.json"))
            if not raw:
                continue
            boxes = prepare_boxes(raw, camera, velo_to_cam, keep_all=keep_all_boxes)
        image_path = os.path.join(kitti360_path, "data_2d_raw", sequence, f"image_{cam_id:02d}",
                                  "data_rect" if cam_id in [0, 1] else "data_rgb", f"{frame:010d}.png")
        if not os.path.isfile(image_path):
            continue
        seg = segmenter(image_loader(image_path) if image_loader else image_path)
        _, masks, colors, boxes_2d, _ = seg
        if masks is None or len(masks) == 0:
            continue
        yield FrameInputs(frame, points, masks, boxes, colors, boxes_2d)


def process_frames(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None,
                   master_csv_path="results/master_car_statistics.csv", frames=None, batch_frames=32,
                   erode_iters=0, v3_pipeline=False, device=0, timestamp=None, read_ahead=True, erosion_kernel_size=3):
    """cvs_erosion.process_frames (cvs_erosion.py:298-379): writes the master CSV and prints the
    overall analysis.  ``segmenter(image) -> (img, masks, colors, boxes, confidences)`` is the
    YOLO stage (unchanged subsystem); pass masks it already eroded, or raw masks plus
    ``erode_iters=1, v3_pipeline=True`` to erode on the GPU.  ``read_ahead=True`` (the default) processes frame
    by frame, as the reference's loop does -- each frame's rows are appended before the next frame is looked at -- with the native
    reader fetching the next scans and parsing the next box files meanwhile; ``read_ahead=False`` reads ``batch_frames`` frames with
    NumPy and runs them as one launch (same CSV; its lines are printed batch by batch).  ``erosion_kernel_size``: the reference's
    knob (cvs_erosion.py:77), as in run_frames -- 5 or 7 is the next experiment after the study's with / without erosion."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if segmenter is None:
        raise ValueError("process_frames needs the segmentation callable (YOLO stays outside this package)")
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    sequence, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    if read_ahead:
        todo = velo.available_frames() if frames is None else list(frames)
        print(f"Found {len(todo)} frames to process")

        box_paths = [os.path.join(root, "bboxes_3D_cam0", f"BBoxes_{f}.json") for f in todo]

        def inputs_for(i, path, scan):
            frame = todo[i]
            # (the box file was parsed by the reader's worker while earlier frames ran: json.load of it was most of a frame's host time)
            boxes = _boxes_of_file(box_paths[i], camera, velo_to_cam, parsed=(scan.boxes_state, scan.box_index, scan.boxes_cam0))
            if boxes is None:
                return None
            image_path = os.path.join(root, "data_2d_raw", sequence, f"image_{cam_id:02d}",
                                      "data_rect" if cam_id in [0, 1] else "data_rgb", f"{frame:010d}.png")
            if not os.path.isfile(image_path):
                return None
            _, masks, colors, _, _ = segmenter(image_loader(image_path) if image_loader else image_path)
            if masks is None or len(masks) == 0:
                return None
            return frame, masks, boxes, colors

        paths = [os.path.join(velo.raw3DPcdPath, "%010d.bin" % f) for f in todo]
        for r in stream_frames(paths, inputs_for, velo_to_rect, camera, 50.0, 10, True, erode_iters, v3_pipeline, device,
                               box_paths=box_paths, announce=lambda i, path: print(f"\nProcessing frame {todo[i]}..."), gather=False,
                               erosion_kernel_size=erosion_kernel_size):
            if r["n_valid"] and r["car_statistics"]:
                append_to_master_csv(r["car_statistics"], r["frame"], master_csv_path, timestamp)
        return analyze_master_csv(master_csv_path)
    items = iter_frame_inputs(root, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames, boxes_as_arrays=True)
    for batch in _batches(items, batch_frames):              # (one batch of scans and masks in memory at a time)
        for r in run_frames(batch, velo_to_rect, camera, 50.0, 10, True, erode_iters, v3_pipeline, device,
                            erosion_kernel_size=erosion_kernel_size):
            if r["n_valid"] == 0:
                continue
            if r["car_statistics"]:
                append_to_master_csv(r["car_statistics"], r["frame"], master_csv_path, timestamp)
    return analyze_master_csv(master_csv_path)


def _depth_map_masks(frames, H, W):
    """The frames' masks as ONE [F,M,H,W] batch for lpf_depth_maps (M = the most masks of a frame; the others pad with empty
    masks) and each frame's own count.  float masks are read as the script's ``mask > 0.5``, uint8 / bool ones as nonzero; a batch
    that mixes them goes as float32 (a nonzero byte is >= 1).  GPU tensors stay on the GPU (the batch is made there).  Masks at
    another size than the camera's raise ValueError: seg_with_pointcloud indexes them with the image's pixels."""
    stacks = []
    for f in frames:
        m = f.masks if f.masks is not None else []
        if _is_device_tensor(m):
            if m.dim() != 3:
                raise ValueError("frame %s: device masks must be [M,H,W], got %s" % (f.frame, tuple(m.shape)))
        elif isinstance(m, np.ndarray):
            if m.ndim != 3 and not (m.ndim == 1 and m.size == 0):
                raise ValueError("frame %s: masks must be [M,H,W], got %s" % (f.frame, m.shape))
        else:
            m = [x if _is_device_tensor(x) else np.asarray(x) for x in m]
            for x in m:
                if x.ndim != 2:
                    raise ValueError("frame %s: each mask must be [H,W], got %s" % (f.frame, tuple(x.shape)))
            if m and any(_is_device_tensor(x) for x in m):
                import torch
                m = torch.stack([x if _is_device_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in m])
            else:
                m = np.stack(m) if m else np.zeros((0, H, W), np.uint8)
        if m.shape[0] and tuple(m.shape[1:]) != (H, W):
            raise ValueError("frame %s: masks must be at the camera's size [M,%d,%d], got %s" % (f.frame, H, W, tuple(m.shape)))
        stacks.append(m)

    def is_float(m):
        return (str(m.dtype) in ("torch.float16", "torch.float32", "torch.float64")) if _is_device_tensor(m) else m.dtype.kind == "f"
    return _padded_mask_batch(stacks, [is_float(m) for m in stacks], (H, W), lambda a: a != 0)


def depth_maps_frames(frames, TrVeloToRect, camera, depth_max=30.0, device=0, ctx=None):
    """seg_with_pointcloud.py:160-170's per-car depth maps of a list of FrameInputs in one native call (lpf_depth_maps) per group
    of up to 256 masks: per frame ``[(car_id, SparseDepthMap)]``, car_id = i + 1 over the frame's masks, each map equal to
    ``per_car_depth_maps``' depthMap (``to_dense()``).  Points: host arrays, Scans of the read-ahead reader or GPU tensors; masks: a
    list, an array or a GPU tensor [M,H,W] at the camera's size, float (> 0.5) or uint8 / bool (nonzero), or ``rle.RleMasks`` (every
    frame of the batch, a frame without masks aside: they go down as runs, nothing dense is made); frames may differ in their mask
    counts.  The depth window is (0, depth_max)."""
    frames = list(frames)
    if not frames:
        return []
    ctx = ctx or get_context(device)
    ctx.set_camera(TrVeloToRect, camera.K, camera.width, camera.height, 0.0, float(depth_max))
    H, W = int(camera.height), int(camera.width)
    compact = _compact_frame_masks(frames, camera, ("rle",))
    rles = compact and compact[1]
    if rles is not None:                                    # run-length masks: the runs go down as they are (lpf_depth_maps_rle),
        batch, Ms, flt = None, [len(r) for r in rles], True       # under depth_maps' default rule
    else:
        batch, Ms, flt = _depth_map_masks(frames, H, W)
    M = max(Ms)
    out = [[] for _ in frames]
    if M == 0:
        return out
    pts = [f.points for f in frames]
    for g in range(0, M, LPF_MAX_MASKS_WIDE):                   # groups of 256 masks, concatenated
        res = ctx.depth_maps(pts, _mask_group(batch, rles, g), binarize="gt0.5" if flt else "astype")
        for f, cars in enumerate(res):
            for j, (pix, dep, pid) in enumerate(cars):
                i = g + j
                if i < Ms[f]:
                    out[f].append((i + 1, SparseDepthMap(i + 1, pix, dep, pid, (H, W))))
    return out


def process_frames_depth_maps(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None, frames=None, depth_max=30.0,
                              device=0):
    """seg_with_pointcloud.projectVeloToImage's frame loop (seg_with_pointcloud.py:105-170) without the plotting: yields
    ``(frame, [(car_id, SparseDepthMap)])`` per frame with detections.  Scans are read in order by the native read-ahead reader; the
    image is data_rect/<frame>.png of the camera (a missing one raises the script's RuntimeError, :145-146);
    ``segmenter(image) -> (img, masks, ...)`` is the segmentation stage (it stays outside this package), and a frame whose masks
    are None or empty prints the script's ``[INFO]`` line and is skipped (:148-151).  cam_id: 0 or 1 (perspective cameras; the
    script runs camera 0)."""
    if segmenter is None:
        raise ValueError("process_frames_depth_maps needs the segmentation callable (YOLO stays outside this package)")
    if cam_id not in (0, 1):
        raise ValueError("cam_id must be 0 or 1 (the perspective cameras), got %r" % (cam_id,))
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    sequence, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    todo = velo.available_frames() if frames is None else list(frames)
    paths = [os.path.join(velo.raw3DPcdPath, "%010d.bin" % f) for f in todo]
    if not paths:
        return
    ctx = get_context(device)
    sizes = [os.path.getsize(p) // 16 for p in paths if os.path.isfile(p)]
    with ScanReader(ctx, paths, n_buffers=3, max_points=max(sizes + [1])) as reader:
        for frame in todo:
            scan = next(reader)
            image_path = os.path.join(root, "data_2d_raw", sequence, "image_%02d" % cam_id,
                                      "data_rect" if cam_id in [0, 1] else "data_rgb", "%010d.png" % frame)
            if not os.path.isfile(image_path):
                raise RuntimeError(f'Image file {image_path} does not exist!')
            seg = segmenter(image_loader(image_path) if image_loader else image_path)
            masks = seg[1] if seg is not None else None
            if masks is None or len(masks) == 0:
                print(f"[INFO] No cars detected in frame {frame}, skipping.")
                continue
            yield frame, depth_maps_frames([FrameInputs(frame, scan, masks)], velo_to_rect, camera, depth_max, device, ctx)[0]


def _overlay_segs(seg_images, n, H, W):
    """The segmented images of depth_overlays_frames as ONE [F,H,W,3] uint8 batch: a NumPy array, or a GPU tensor when any image is
    one.  An image that is not uint8 [H,W,3] at the camera's size raises ValueError (seg_with_pointcloud.py:178 would fail)."""
    segs = list(seg_images)
    if len(segs) != n:
        raise ValueError("one segmented image per frame: %d frames, %d images" % (n, len(segs)))
    for i, s in enumerate(segs):
        dt = str(s.dtype) if _is_device_tensor(s) else np.asarray(s).dtype.name
        if tuple(s.shape) != (H, W, 3) or dt not in ("uint8", "torch.uint8"):
            raise ValueError("segmented image %d must be uint8 [%d,%d,3] at the camera's size, got %s %s" % (i, H, W, dt, tuple(s.shape)))
    if any(_is_device_tensor(s) for s in segs):
        import torch
        dev = next(s.device for s in segs if _is_device_tensor(s))
        return torch.stack([s.to(dev) if _is_device_tensor(s) else torch.from_numpy(np.ascontiguousarray(s)).to(dev) for s in segs])
    return np.stack([np.asarray(s) for s in segs]) if segs else np.zeros((0, H, W, 3), np.uint8)


def depth_overlays_frames(frames, seg_images, TrVeloToRect, camera, depth_max=30.0, device=0, ctx=None):
    """seg_with_pointcloud.py:160-180 for a list of FrameInputs: per frame ``[(car_id, SparseDepthMap, overlay)]`` for the cars with
    at least one pixel, in the script's car order.  ``overlay`` is uint8 [H,W,3], the script's image_withseg after
    cv2.cvtColor(RGB2BGR) byte for byte (a NumPy array, or a GPU tensor when the segmented images are on the GPU).  seg_images: one
    uint8 [H,W,3] segmented image per frame (the segmenter's first result) at the camera's size.  The depth maps come from
    depth_maps_frames (ragged mask counts, groups of 256 masks), the overlays from one lpf_depth_overlays call per group of up to
    256 nonzero cars per frame.  The depth window is (0, depth_max)."""
    frames = list(frames)
    H, W = int(camera.height), int(camera.width)
    segs = _overlay_segs(seg_images, len(frames), H, W)
    if not frames:
        return []
    ctx = ctx or get_context(device)
    maps = depth_maps_frames(frames, TrVeloToRect, camera, depth_max, device, ctx)
    cars = [[(cid, sm) for cid, sm in fr if len(sm)] for fr in maps]      # the script's `if np.max(depthMap) == 0: continue`
    out = [[] for _ in frames]
    for g in range(0, max(len(c) for c in cars), LPF_MAX_MASKS_WIDE):
        part = [c[g:g + LPF_MAX_MASKS_WIDE] for c in cars]
        M = max(len(c) for c in part)
        empty = (np.zeros(0, np.int64), np.zeros(0, np.float64))
        lists = [[(sm.pixels, sm.depth) for _, sm in c] + [empty] * (M - len(c)) for c in part]
        images, _ = ctx.depth_overlays(lists, segs)
        for f, c in enumerate(part):
            for j, (cid, sm) in enumerate(c):
                out[f].append((cid, sm, images[f, j]))
    return out


def process_frames_depth_overlays(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None, frames=None, depth_max=30.0,
                                  device=0):
    """process_frames_depth_maps' frame loop (seg_with_pointcloud.py:105-180) with the overlays: yields ``(frame, [(car_id,
    SparseDepthMap, overlay)])`` per frame with detections, overlay = the image the script draws in its lower panel (:188), from the
    segmenter's image ``seg[0]``.  Cars without a pixel are left out, as the script skips them (:174-175).  The figure and PNG writing
    stay outside this package."""
    if segmenter is None:
        raise ValueError("process_frames_depth_overlays needs the segmentation callable (YOLO stays outside this package)")
    if cam_id not in (0, 1):
        raise ValueError("cam_id must be 0 or 1 (the perspective cameras), got %r" % (cam_id,))
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    sequence, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    todo = velo.available_frames() if frames is None else list(frames)
    paths = [os.path.join(velo.raw3DPcdPath, "%010d.bin" % f) for f in todo]
    if not paths:
        return
    ctx = get_context(device)
    sizes = [os.path.getsize(p) // 16 for p in paths if os.path.isfile(p)]
    with ScanReader(ctx, paths, n_buffers=3, max_points=max(sizes + [1])) as reader:
        for frame in todo:
            scan = next(reader)
            image_path = os.path.join(root, "data_2d_raw", sequence, "image_%02d" % cam_id,
                                      "data_rect" if cam_id in [0, 1] else "data_rgb", "%010d.png" % frame)
            if not os.path.isfile(image_path):
                raise RuntimeError(f'Image file {image_path} does not exist!')
            seg = segmenter(image_loader(image_path) if image_loader else image_path)
            masks = seg[1] if seg is not None else None
            if masks is None or len(masks) == 0:
                print(f"[INFO] No cars detected in frame {frame}, skipping.")
                continue
            yield frame, depth_overlays_frames([FrameInputs(frame, scan, masks)], [seg[0]], velo_to_rect, camera, depth_max, device,
                                               ctx)[0]


def process_frames_multicam(seq=0, cam_ids=(0, 1), segmenter=None, image_loader=None, kitti360_path=None, master_csv_paths=None,
                            frames=None, erode_iters=0, v3_pipeline=False, device=0, timestamp=None, erosion_kernel_size=3):
    """process_frames for several perspective cameras of the rig at once: each scan is read once (the native read-ahead reader) and
    each box file parsed once; per frame the segmenter runs on every camera's image and ONE pass (run_frames_multicam) labels the scan
    in all of them.  Camera c's boxes are prepared with camera c's TrVeloToCam and visibility filter, as the reference does for
    ``cam_id = c`` (V3:532-535, 561-562: the cam-0 corners go through the selected camera's transform).  Camera c's rows go to
    ``master_csv_paths[c]`` (default ``results/master_car_statistics_cam<c>.csv``), byte for byte what
    ``process_frames(seq, cam_id=c, ...)`` writes with the same arguments and timestamp.  Skip rules per the reference: a frame without
    a box file (or with an empty one) is skipped for every camera -- the reference skips before it looks at an image; a missing image
    or no detections skip only that camera's part of the frame.  Returns ``{cam_id: analyze_master_csv(path)}``.
    ``erosion_kernel_size``: as in run_frames."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if segmenter is None:
        raise ValueError("process_frames_multicam needs the segmentation callable (YOLO stays outside this package)")
    cam_ids = [int(c) for c in cam_ids]
    if not 1 <= len(cam_ids) <= LPF_MAX_CAMS or len(set(cam_ids)) != len(cam_ids) or any(c not in (0, 1) for c in cam_ids):
        raise ValueError("cam_ids: 1 to %d distinct perspective cameras (0, 1), got %r" % (LPF_MAX_CAMS, cam_ids))
    if master_csv_paths is None:
        master_csv_paths = {c: "results/master_car_statistics_cam%d.csv" % c for c in cam_ids}
    elif not isinstance(master_csv_paths, dict):
        master_csv_paths = dict(zip(cam_ids, master_csv_paths))
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    setups = {c: sequence_setup(root, seq, c) for c in cam_ids}
    sequence, _, _, _, velo = setups[cam_ids[0]]
    todo = velo.available_frames() if frames is None else list(frames)
    print(f"Found {len(todo)} frames to process")
    box_paths = [os.path.join(root, "bboxes_3D_cam0", f"BBoxes_{f}.json") for f in todo]
    scan_paths = [os.path.join(velo.raw3DPcdPath, "%010d.bin" % f) for f in todo]
    sizes = [os.path.getsize(p) // 16 for p in scan_paths if os.path.isfile(p)]
    ctx = get_context(device)
    with ScanReader(ctx, scan_paths, n_buffers=3, max_points=max(sizes + [1]), box_paths=box_paths) as reader:
        for i, frame in enumerate(todo):
            print(f"\nProcessing frame {frame}...")
            try:
                scan = next(reader)
            except RuntimeError as e:
                print(f"Failed to load frame {os.path.basename(scan_paths[i])}: {e}")
                continue
            parsed = (scan.boxes_state, scan.box_index, scan.boxes_cam0)
            inputs, cams = {}, {}
            for c in cam_ids:
                _, camera, velo_to_cam, velo_to_rect, _ = setups[c]
                boxes = _boxes_of_file(box_paths[i], camera, velo_to_cam, parsed=parsed)
                if boxes is None:                        # (no box file: the same for every camera -- the frame is skipped)
                    break
                image_path = os.path.join(root, "data_2d_raw", sequence, f"image_{c:02d}", "data_rect", f"{frame:010d}.png")
                if not os.path.isfile(image_path):
                    continue
                _, masks, colors, _, _ = segmenter(image_loader(image_path) if image_loader else image_path)
                if masks is None or len(masks) == 0:
                    continue
                inputs[c] = FrameInputs(frame, scan, masks, boxes, colors)
                cams[c] = (velo_to_rect, camera)
            if not inputs:
                continue
            order = list(inputs)
            res = run_frames_multicam([[inputs[c]] for c in order], [cams[c] for c in order], 50.0, 10, True, erode_iters, v3_pipeline,
                                      device, ctx, gather_scans=False, erosion_kernel_size=erosion_kernel_size)
            for c, r in zip(order, res):
                r = r[0]
                if r["n_valid"] and r["car_statistics"]:
                    append_to_master_csv(r["car_statistics"], r["frame"], master_csv_paths[c], timestamp)
    return {c: analyze_master_csv(master_csv_paths[c]) for c in cam_ids}


def process_frame_with_statistics(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None,
                                  visualizer=None, frames=None, erode_iters=0, v3_pipeline=False, device=0, v3_keys=False,
                                  erosion_kernel_size=3):
    """V3's entry point (V3:516-641) without the blocking Open3D window: per frame it prints the
    statistics table and hands (frame, car_statistics, points_valid, bg_assigned) to
    ``visualizer`` when one is given.  bg_assigned is V4's vectorised form of V3:609-616.  ``v3_keys=True``: the statistics carry
    V3's own key set -- corners_velo, inside_mask, car_points (car_statistics_v3_frames) -- and each result ``inside_parts``, from
    which inside_outside_cloud_frames builds V3's cloud; the default leaves them out, as cvs_erosion's dicts do.
    ``erosion_kernel_size``: as in run_frames (V3:55)."""
    erosion_kernel_size = _erosion_kernel_size(erosion_kernel_size)
    if segmenter is None:
        raise ValueError("process_frame_with_statistics needs the segmentation callable")
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    _, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    items = collect_frame_inputs(root, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames)
    results = []
    run = car_statistics_v3_frames if v3_keys else run_frames
    for r, item in zip(run(items, velo_to_rect, camera, 50.0, 10, True, erode_iters, v3_pipeline, device,
                           erosion_kernel_size=erosion_kernel_size), items):
        if r["n_valid"] == 0:
            continue
        print_summary_statistics(r["car_statistics"])
        if visualizer is not None:
            visualizer(r["frame"], r["car_statistics"], r["points_valid"], r["bg_assigned"])
        results.append(r)
    return results


def process_frame(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None, visualizer=None,
                  frames=None, device=0):
    """V4's entry point (V4:213-336): depth < 30 clip, per-mask point sets, ``bg_assigned`` and the
    2D-IoU box matching; the Open3D window is replaced by the optional ``visualizer`` callable,
    which receives (frame, car_point_sets, colors, remaining_points, matched_pairs)."""
    if segmenter is None:
        raise ValueError("process_frame needs the segmentation callable")
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    _, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    items = collect_frame_inputs(root, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames)
    results = []
    # the 2D matching of every frame in one lpf_match_2d call (it reads the detections and the boxes' rectangles only)
    pairs = match_detections_frames([i.boxes_2d for i in items], [i.bboxes_3d for i in items], [i.colors for i in items], camera,
                                    device=device)
    for r, item, matched in zip(run_frames(items, velo_to_rect, camera, 30.0, 10, True, 0, False, device), items, pairs):
        if r["n_valid"] == 0:
            continue
        r["remaining_points"] = r["points_valid"][~r["bg_assigned"]]
        r["matched_pairs"] = matched
        print(f"Visualizing frame {r['frame']} with {sum(len(s) > 0 for s in r['car_point_sets']) + 1 + len(r['matched_pairs'])} objects")
        if visualizer is not None:
            visualizer(r["frame"], r["car_point_sets"], item.colors, r["remaining_points"], r["matched_pairs"])
        results.append(r)
    return results


def projectVeloToImage(seq=0, cam_id=0, segmenter=None, image_loader=None, kitti360_path=None, visualizer=None,
                       frames=None, device=0, assign="host"):
    """V5's entry point (V5:419-571): every annotated box (no visibility filter), depth < 30 clip,
    per-mask point sets, ``bg_assigned`` and the score + Hungarian box matching; ``visualizer`` receives
    (frame, car_point_sets, colors, remaining_points, matched_pairs) instead of the Open3D window.  assign: where the Hungarian
    assignment runs, "host" (scipy) or "device" (lpf_assign_2d), as improved_match_detections_frames'."""
    _assign_route(assign)
    if segmenter is None:
        raise ValueError("projectVeloToImage needs the segmentation callable")
    root = kitti360_path or os.environ["KITTI360_DATASET"]
    _, camera, velo_to_cam, velo_to_rect, velo = sequence_setup(root, seq, cam_id)
    items = collect_frame_inputs(root, seq, cam_id, segmenter, image_loader, camera, velo_to_cam, velo, frames,
                                 keep_all_boxes=True)
    results = []
    # the pair scores of every frame in one lpf_match_2d call; the assignment and its printed lines stay in the frame's turn
    scores = _improved_scores([i.boxes_2d for i in items], [i.bboxes_3d for i in items], camera, device=device, assign=assign)
    for r, item, sc in zip(run_frames(items, velo_to_rect, camera, 30.0, 10, True, 0, False, device), items, scores):
        print(f"[DEBUG] Frame {r['frame']}: {r['n_valid']} points passed validation filter")
        if r["n_valid"] == 0:
            print(f"[WARN] No valid LiDAR points in frame {r['frame']}")
            continue
        r["remaining_points"] = r["points_valid"][~r["bg_assigned"]]
        r["matched_pairs"] = _improved_assign(item.boxes_2d, item.bboxes_3d, item.colors, sc)
        if visualizer is not None:
            visualizer(r["frame"], r["car_point_sets"], item.colors, r["remaining_points"], r["matched_pairs"])
        results.append(r)
    return results
