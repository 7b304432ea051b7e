"""NumPy restatement of the reference's 2D matching arithmetic, type for type -- the yardstick of lpf_match_2d for batches the scalar
functions (pipeline.calculate_iou_2d / calculate_matching_score / match_detections_to_bboxes) are too slow for.

The detector's boxes are float32: iterating them gives np.float32 scalars.  A projected box holds np.int64 pixels in the reference and
the same values as float64 here; under NumPy 2 promotion float32 (op) int64 / float64 is float64 while float32 (op) float32 stays
float32, and Python's max(a, b) / min(a, b) return b only when it is strictly greater / smaller.  So, with T the detections' dtype:
  xa = box x0 if box x0 > det x1 else det x1;  xb = box x1 if box x1 < det x2 else det x2;  same for y;  iou 0.0 if xb <= xa or yb <= ya
  xb - xa is a T subtraction when both ends are the detection's, else float64;  the product of the differences is a T product only when
  both are T;  area1 = (x2 - x1) * (y2 - y1) in T, area2 float64;  union = area1 + area2 - inter (float64, left to right)
  detection centre in T, box centre float64;  dist = sqrt(fma(dy, dy, dx * dx)): np.linalg.norm of the 2-vector is BLAS dot, which
  fuses the second product into the sum;  center_score = c if c > 0 else 0, c = 1 - dist / 1000
  size_score = min(area1, area2) / max(area1, area2) if both > 0 else 0;  total = w_iou iou + w_center centre + w_size size; cost = 1 - total
  equal areas: min and max both return the detection's area1, the ratio is a T 1.0 and the Python float w_size times it is a T product
  (a Python float is "weak" under NumPy 2 promotion): the size term is T(w_size), not w_size
tests/test_match2d_api.py holds this file against the scalar functions bit for bit."""
import numpy as np

F64 = np.float64


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p + e = a * b exactly (Veltkamp / Dekker; no overflow or underflow for the magnitudes of pixel coordinates)"""
    p = a * b
    c = 134217729.0                                         # 2^27 + 1
    ah = a * c
    ah = ah - (ah - a)
    al = a - ah
    bh = b * c
    bh = bh - (bh - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, element-wise on float64 arrays: the exact product as p + e, the exact sum p + c as s + t,
    then t + e rounded to odd before the last addition (Boldo & Melquiond: a sum through round-to-odd rounds like the exact sum)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F64), np.asarray(b, F64), np.asarray(c, F64))
    p, e = _two_prod(a, b)
    s, t = _two_sum(p, c)
    u, v = _two_sum(t, e)
    bits = u.view(np.int64)
    even = (bits & 1) == 0
    away = np.where(v > 0, np.inf, -np.inf)
    u = np.where((v != 0) & even, np.nextafter(u, away), u)
    return s + u


def score(dets, bbox2d, front=None, weights=(0.5, 0.3, 0.2)):
    """dict of float64 [D,B] matrices iou, center, size, total, cost for detections [D,4] (float32 or float64: T) against projected
    boxes float64 [B,4]; a column whose front is 0 is iou 0, scores 0, cost 1."""
    dets = np.asarray(dets)
    T = dets.dtype.type
    assert T in (np.float32, np.float64)
    bb = np.asarray(bbox2d, F64).reshape(-1, 4)
    D, B = len(dets), len(bb)
    x1, y1, x2, y2 = (dets[:, k][:, None] for k in range(4))
    bx0, by0, bx1, by1 = (bb[:, k][None, :] for k in range(4))
    up = lambda a: a.astype(F64)
    with np.errstate(all="ignore"):
        xa_box, xb_box, ya_box, yb_box = bx0 > up(x1), bx1 < up(x2), by0 > up(y1), by1 < up(y2)
        xa, xb = np.where(xa_box, bx0, up(x1)), np.where(xb_box, bx1, up(x2))
        ya, yb = np.where(ya_box, by0, up(y1)), np.where(yb_box, by1, up(y2))
        empty = (xb <= xa) | (yb <= ya)
        wT, hT = x2 - x1, y2 - y1                           # T
        wt, ht = ~xa_box & ~xb_box, ~ya_box & ~yb_box
        w, h = np.where(wt, up(wT), xb - xa), np.where(ht, up(hT), yb - ya)
        area1 = wT * hT                                     # T
        inter = np.where(wt & ht, up(area1), w * h)
        area2 = (bx1 - bx0) * (by1 - by0)
        union = (up(area1) + area2) - inter
        ok = ~empty & (union > 0)
        iou = np.where(ok, inter / np.where(ok, union, 1.0), 0.0)
        cdx, cdy = (x1 + x2) / T(2), (y1 + y2) / T(2)       # T
        dx, dy = up(cdx) - (bx0 + bx1) / 2, up(cdy) - (by0 + by1) / 2
        c = 1 - np.sqrt(fma(dy, dy, dx * dx)) / 1000
        center = np.where(c > 0, c, 0.0)
        a1 = np.broadcast_to(up(area1), (D, B))
        a2 = np.broadcast_to(area2, (D, B))
        lo, hi = np.where(a2 < a1, a2, a1), np.where(a2 > a1, a2, a1)
        both = (a1 > 0) & (a2 > 0)
        size = np.where(both, lo / np.where(both, hi, 1.0), 0.0)
        term = np.where(both & (a1 == a2), F64(T(weights[2]) * T(1)), weights[2] * size)
        total = (weights[0] * iou + weights[1] * center) + term
        cost = 1 - total
    out = {"iou": iou, "center": center, "size": size, "total": total, "cost": cost}
    out = {k: np.array(np.broadcast_to(v, (D, B)), dtype=F64) for k, v in out.items()}
    if front is not None:
        gone = np.asarray(front) <= 0
        for k in out:
            out[k][:, gone] = 1.0 if k == "cost" else 0.0
    return out


def best(iou, min_iou=0.25):
    """V4:170-178 on an IoU matrix [D,B]: (best_box int32 [D], best_iou float64 [D]) -- the first strict maximum in list order among
    the columns with iou > min_iou (and > 0: the scan starts from best_iou = 0), -1 / 0 if none."""
    D, B = iou.shape
    if B == 0:
        return np.full(D, -1, np.int32), np.zeros(D, F64)
    j = np.argmax(iou, axis=1)                              # (argmax: the first of equal maxima)
    v = iou[np.arange(D), j]
    won = (v > 0) & (v > min_iou)
    return np.where(won, j, -1).astype(np.int32), np.where(won, v, 0.0)


def match(dets, bbox2d, front, min_iou=0.25, weights=(0.5, 0.3, 0.2)):
    """everything lpf_match_2d returns for one frame"""
    out = score(dets, bbox2d, front, weights)
    out["best_box"], out["best_iou"] = best(out["iou"], min_iou)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the seeded generator of tests/test_match2d_api.py and tests/test_gpu_match2d.py -------------------------------------------
def cases(seed, D, B, dtype=np.float32, fraction=False):
    """(dets [D,4] dtype, bbox2d float64 [B,4] integer-valued, front int32 [B]): detections crowded into a part of a 1408 x 376 image
    (so that a good share of all pairs overlaps), boxes
    built from the detections so that on each axis the intersection's lower edge comes from the detection or the box and its upper
    edge from the detection or the box -- alone and combined over the two axes --, with duplicated boxes (ties), boxes equal to their
    detection, zero-area boxes and detections, boxes beside their detection and boxes with front == 0.  ``fraction``: the detections
    get non-integer coordinates (the detector's are)."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(520, 700, D).astype(F64)
    y1 = rng.integers(120, 180, D).astype(F64)
    w = rng.integers(8, 200, D).astype(F64)
    h = rng.integers(8, 76, D).astype(F64)
    if fraction:
        x1, y1, w, h = x1 + rng.random(D), y1 + rng.random(D), w + rng.random(D), h + rng.random(D)
    dets = np.stack([x1, y1, x1 + w, y1 + h], 1)
    if D:
        z = rng.random(D) < 0.04
        dets[z, 2] = dets[z, 0]                             # zero-width detections
        z = rng.random(D) < 0.02
        dets[z, 2], dets[z, 0] = dets[z, 0].copy(), dets[z, 2].copy()       # x2 < x1
    dets = dets.astype(dtype)
    bb = np.zeros((B, 4), F64)
    front = np.full(B, 8, np.int32)
    for j in range(B):
        kind = rng.integers(0, 12)
        if D == 0 or kind == 0:                             # unrelated
            a, b = rng.integers(300, 900), rng.integers(0, 300)
            bb[j] = [a, b, a + rng.integers(1, 300), b + rng.integers(1, 120)]
            continue
        d = np.floor(dets[rng.integers(0, D)].astype(F64))
        if kind == 1:                                       # equal to (the floor of) its detection
            bb[j] = d
        elif kind == 2 and j > 0:                           # a duplicate: ties
            bb[j] = bb[rng.integers(0, j)]
        elif kind == 3:                                     # zero area
            bb[j] = [d[0] + 2, d[1] + 2, d[0] + 2, d[3]]
        elif kind == 4:                                     # beside its detection (touching: xb == xa)
            bb[j] = [d[2], d[1], d[2] + 40, d[3]]
        else:                                               # each edge inside (the box's) or outside (the detection's), per axis
            lo_x, hi_x, lo_y, hi_y = rng.integers(0, 2, 4)
            mx, my = max(1.0, np.floor((d[2] - d[0]) / 4)), max(1.0, np.floor((d[3] - d[1]) / 4))
            bb[j] = [d[0] + mx if lo_x else d[0] - rng.integers(0, 30), d[1] + my if lo_y else d[1] - rng.integers(0, 30),
                     d[2] - mx if hi_x else d[2] + rng.integers(0, 30), d[3] - my if hi_y else d[3] + rng.integers(0, 30)]
    front[rng.random(B) < 0.08] = 0
    return dets, bb, front


# ---- the scalar functions as matrices, and the comparison rule for values that depend on the BLAS behind np.linalg.norm --------
def scalar_scores(dets, bbox2d, front, score_fn, iou_fn):
    """The [D,B] matrices from a scalar calculate_matching_score / calculate_iou_2d (this package's or the reference's), fed as V5 feeds
    them: np scalars of the detections' dtype, float64 rectangles; columns with front == 0 are iou 0, scores 0, cost 1."""
    D, B = len(dets), len(bbox2d)
    out = {k: np.zeros((D, B)) for k in ("iou", "center", "size", "total", "cost")}
    out["cost"][:] = 1.0
    for i, box in enumerate(dets):
        x1, y1, x2, y2 = box
        d = {"bbox": [x1, y1, x2, y2], "center": [(x1 + x2) / 2, (y1 + y2) / 2], "size": [x2 - x1, y2 - y1], "area": (x2 - x1) * (y2 - y1)}
        for j in range(B):
            if front[j] <= 0:
                continue
            x0, y0, xx, yy = bbox2d[j]
            info = {"bbox": [x0, y0, xx, yy], "center": [(x0 + xx) / 2, (y0 + yy) / 2], "size": [xx - x0, yy - y0], "area": (xx - x0) * (yy - y0)}
            total, det = score_fn(d, info)
            assert det["iou"] == iou_fn([x1, y1, x2, y2], [x0, y0, xx, yy])
            out["iou"][i, j], out["center"][i, j], out["size"][i, j], out["total"][i, j] = det["iou"], det["center_score"], det["size_score"], total
            out["cost"][i, j] = 1 - total
    return out


BLAS_BOUND = 2.0 ** -48


def compare_scores(got, exp, what):
    """IoU and size score bit for bit.  Centre, total and cost bit for bit too -- unless the machine that made ``exp`` computes
    np.linalg.norm of a 2-vector with another correctly rounded form than the fused one: two such forms differ by at most one ulp of the
    distance, below 2^-40 for a distance under 4096 (at 4096 or more both give a centre score of exactly 0), which after / 1000, 1 -
    and the weighted sum (values below 4, three more roundings) stays under 2^-48 absolute.  Returns True when the clause was needed."""
    for k in ("iou", "size"):
        assert same_bits(got[k], exp[k]), "%s: %s differs (max %g)" % (what, k, np.abs(np.asarray(got[k]) - np.asarray(exp[k])).max())
    needed = False
    for k in ("center", "total", "cost"):
        if same_bits(got[k], exp[k]):
            continue
        err = float(np.abs(np.asarray(got[k], F64) - np.asarray(exp[k], F64)).max())
        assert err <= BLAS_BOUND, ("%s: %s differs by %g, more than 2^-48: this is NOT the case of another correctly rounded centre distance "
                                   "(np.linalg.norm's BLAS), the arithmetic itself differs" % (what, k, err))
        needed = True
    return needed
