"""One small, seeded, ragged batch per batched analysis call -- lpf_match_2d, lpf_assign_costs, lpf_assign_2d, lpf_inside_masks,
lpf_box_points, lpf_box_views, lpf_first_match, lpf_depth_maps, lpf_depth_overlays -- for the tests of their SECOND and later ranges
(tests/test_gpu_batch_ranges.py; checked on the CPU by tests/test_batch_range_cases.py).  Every batch has empty frames first, last and
in the middle, a frame without detections next to one without boxes, and distinct inputs in every frame, so that a frame's outputs
identify it: a kernel that enters range 2 with range 1's base gives another answer, and compare() sees it.

A case holds its inputs, the reference outputs in the layout the C call writes them (from the per-call restatements: match2d_ref,
assign_ref / SciPy, inside_ref, box_points_ref, box_views_ref, first_match_ref, the depth-map definition on the oracle's depth image,
overlay_ref) and, per output, the rows of every plan item: spans[name][i] .. spans[name][i + 1] are item i's rows along axis 0.  What
a call leaves alone -- host rows beyond a frame's count, rows of a frame whose lists did not fit -- holds the sentinel fill[name] in
the reference, so compare(), which is bit-exact on whole arrays, checks the sentinels too.  Nothing here imports a GPU module."""
import functools

import numpy as np

import assign_ref as A
import box_points_ref as BP
import box_views_ref as BV
import first_match_ref as FM
import inside_ref as IR
import match2d_ref as M2
import overlay_ref as OV
import projection_cases as PC
from conftest import load_calib

CALLS = ("match_2d", "assign_costs", "assign_2d", "inside_masks", "box_points", "box_views", "first_match", "depth_maps", "depth_overlays")
# (detections, boxes) per frame: empty frames first, in the middle and last; no detections next to no boxes
SHAPES = ((0, 0), (3, 4), (5, 2), (0, 3), (4, 0), (7, 6), (2, 9), (0, 0), (6, 6), (1, 1), (9, 3), (3, 7), (4, 4), (0, 0))
F = len(SHAPES)
POINTS = (0, 300, 517, 64, 0, 1100, 255, 700, 0, 33, 1025, 410, 129, 0)      # points per frame: across 64, 256, 1024; empties as above
BOXES = (0, 2, 3, 0, 1, 3, 2, 3, 0, 1, 2, 3, 3, 0)                           # boxes per frame of the calls on the boxes in force
DMAX = 30.0
MIN_IOU, WEIGHTS = 0.1, (0.5, 0.3, 0.2)
MIN_POINTS = 4
OVERFLOW_FRAME = 10                                   # lpf_inside_masks: the frame whose lists do not fit inst_cap


class Case:
    """call: the call's name; items: what its ranges count (frames, or images for depth_overlays); inputs: dict; ref / spans / fill:
    see the module's text; frame_kind: the outputs that hold one row per item (the others hold an item's detections, boxes, pairs,
    points or list rows); nonempty: bool [items], the items that have rows in some per-item output."""

    def __init__(self, call, items, inputs, ref, spans, fill, frame_kind):
        self.call, self.items, self.inputs, self.ref, self.spans, self.fill = call, int(items), inputs, ref, spans, fill
        self.frame_kind = tuple(frame_kind)
        for k, r in ref.items():
            r.setflags(write=False)
            s = spans[k]
            assert len(s) == self.items + 1 and s[0] == 0 and s[-1] == len(r) and (np.diff(s) >= 0).all(), (call, k)
        self.item_kind = tuple(k for k in ref if k not in self.frame_kind)
        self.nonempty = np.zeros(self.items, bool)
        for k in self.item_kind:
            self.nonempty |= np.diff(spans[k]) > 0

    def rows(self, name, item):
        s = self.spans[name]
        return self.ref[name][int(s[item]):int(s[item + 1])]

    def host_bytes(self):
        """the bytes of the case's array inputs and outputs: what a call with every array in host memory stages, roughly"""
        n = sum(v.nbytes for v in self.ref.values())
        for v in self.inputs.values():
            for a in (v if isinstance(v, (list, tuple)) else [v]):
                n += a.nbytes if isinstance(a, np.ndarray) else 0
        return n


def compare(got, ref):
    """None when every output of ``got`` is the reference's, bit for bit (dtype, size and bytes; ``got`` may hold an output in another
    shape of the same size, e.g. [F, M] for [F * M]) -- else a line that names the first output and row that differ."""
    for k, r in ref.items():
        if k not in got:
            return "%s is missing" % k
        g = np.ascontiguousarray(got[k])
        if g.dtype != r.dtype or g.size != r.size:
            return "%s: %s %s, expected %s %s" % (k, g.dtype, g.shape, r.dtype, r.shape)
        g = g.reshape(r.shape)
        if g.tobytes() != r.tobytes():
            w = max(r.size // max(len(r), 1), 1) * r.itemsize
            a, b = np.frombuffer(g.tobytes(), np.uint8).reshape(-1, w), np.frombuffer(r.tobytes(), np.uint8).reshape(-1, w)
            row = int(np.flatnonzero((a != b).any(axis=1))[0])
            return "%s: row %d of %d differs" % (k, row, len(r))
    return None


def forge(case, cut, kind, clear=False, fill=None):
    """The answer a wrong base would give: the rows of range 2 -- items cut .. -- of every output of ``kind`` ("item" or "frame")
    written with range 1's base, i.e. from the array's first row on.  clear: range 2's own rows hold the fill instead (nothing wrote
    them; ``fill``: other sentinels than the case's).  None when range 2 has no row of that kind, or range 1 none (both bases are then the array's first row)."""
    out = {k: np.array(v) for k, v in case.ref.items()}
    any_rows = False
    for k in (case.item_kind if kind == "item" else case.frame_kind):
        s = case.spans[k]
        a, e = int(s[cut]), int(s[-1])
        if e == a or a == 0:
            continue
        any_rows = True
        if clear:
            out[k][a:e] = (fill or case.fill)[k]
        out[k][:e - a] = case.ref[k][a:e]
    return out if any_rows else None


def _off(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _cat(parts, dtype, tail=()):
    parts = [np.asarray(p, dtype).reshape((-1,) + tuple(tail)) for p in parts]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0,) + tuple(tail), dtype)


# ---- lpf_match_2d, lpf_assign_costs, lpf_assign_2d ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pairs_data():
    data = [M2.cases(500 + i, d, b, np.float32, fraction=bool(i % 2)) for i, (d, b) in enumerate(SHAPES)]
    return [d[0] for d in data], [d[1] for d in data], [np.asarray(d[2], np.int32) for d in data]


@functools.lru_cache(maxsize=None)
def match_2d():
    dets, bbs, fronts = _pairs_data()
    refs = [M2.match(d, b, f, MIN_IOU, WEIGHTS) for d, b, f in zip(dets, bbs, fronts)]
    D, B = np.array([s[0] for s in SHAPES]), np.array([s[1] for s in SHAPES])
    ref = {"best_box": _cat([r["best_box"] for r in refs], np.int32), "best_iou": _cat([r["best_iou"] for r in refs], np.float64)}
    for k in ("iou", "center", "size", "total", "cost"):
        ref[k] = _cat([r[k] for r in refs], np.float64)
    spans = {k: _off(D) if k.startswith("best") else _off(D * B) for k in ref}
    fill = {"best_box": -1, "best_iou": 0.0, "iou": 0.0, "center": 0.0, "size": 0.0, "total": 0.0, "cost": 0.0}
    return Case("match_2d", F, dict(dets=dets, bbox2d=bbs, front=fronts), ref, spans, fill, ())


STATUS = {5: 1, 10: 2, 12: 1}                         # lpf_assign_costs: frames with a NaN, with no finite entry, with a -inf


@functools.lru_cache(maxsize=None)
def assign_costs():
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(41)
    costs, fronts = [], []
    for i, (d, b) in enumerate(SHAPES):
        m = A.matrix(rng, A.KINDS[i % len(A.KINDS)], d, b) + (i / 64.0 if d * b else 0.0)
        fr = np.ones(b, np.int32)
        if i == 5:
            m[2, 3] = np.nan
        if i == 10:
            m[:] = np.inf
        if i == 12:
            m[0, 1] = -np.inf
        if i == 6:
            fr[::3] = 0                               # a third of the columns has no projection
        if i == 8:
            fr[:] = 0                                 # every column dropped: nothing is assigned, status 0
        costs.append(m)
        fronts.append(fr)
    col, status = [], np.zeros(F, np.int32)
    for i, (m, fr) in enumerate(zip(costs, fronts)):
        c = np.full(m.shape[0], -1, np.int32)
        live = np.flatnonzero(fr > 0)
        st = A.solve_front(m, fr)[0] if m.shape[0] and len(live) else A.OK
        status[i] = st
        assert st == STATUS.get(i, 0), i
        if st == A.OK and m.shape[0] and len(live):
            r, cc = linear_sum_assignment(m[:, live])
            c[r] = live[cc]
        col.append(c)
    D = np.array([s[0] for s in SHAPES])
    ref = {"col_of_row": _cat(col, np.int32), "status": status}
    spans = {"col_of_row": _off(D), "status": np.arange(F + 1, dtype=np.int64)}
    return Case("assign_costs", F, dict(costs=costs, front=fronts), ref, spans, {"col_of_row": -1, "status": 0}, ("status",))


ASSIGN2D_ROWS = ("box_of_det", "iou", "center", "size", "total", "accepted")


def assign2d_frame(d, b, fr):
    """lpf_assign_2d's rows of one frame: SciPy's assignment on match2d_ref's cost of the boxes with front > 0, the scores of the
    assigned pairs and V5's thresholds (0.3 on the total, 0.15 on the IoU)"""
    from scipy.optimize import linear_sum_assignment
    n = len(d)
    sc = M2.score(d, b, fr, WEIGHTS)
    live = np.flatnonzero(np.asarray(fr) > 0)
    out = dict(box_of_det=np.full(n, -1, np.int32), accepted=np.zeros(n, np.int32), iou=np.zeros(n), center=np.zeros(n), size=np.zeros(n),
               total=np.zeros(n))
    if n and len(live):
        assert A.solve(sc["cost"][:, live])[0] == 0          # (the scores of finite weights hold no NaN and no infinity: always solvable)
        r, c = linear_sum_assignment(sc["cost"][:, live])
        box = out["box_of_det"]
        box[r] = live[c]
        for k in ("iou", "center", "size", "total"):
            out[k][r] = sc[k][r, box[r]]
        out["accepted"][r] = (sc["total"][r, box[r]] >= 0.3) & (sc["iou"][r, box[r]] >= 0.15)
    return out


@functools.lru_cache(maxsize=None)
def assign_2d():
    dets, bbs, fronts = _pairs_data()
    dets, fronts = [np.array(d) for d in dets], [np.array(f) for f in fronts]
    fronts[8][:] = 0                                  # every box of frame 8 has no projection
    per = {k: [] for k in ASSIGN2D_ROWS}
    status = np.zeros(F, np.int32)
    for i, (d, b, fr) in enumerate(zip(dets, bbs, fronts)):
        r = assign2d_frame(d, b, fr)
        for k in ASSIGN2D_ROWS:
            per[k].append(r[k])
    names = ASSIGN2D_ROWS
    D = np.array([s[0] for s in SHAPES])
    ref = {k: _cat(per[k], np.int32 if k in ("box_of_det", "accepted") else np.float64) for k in names}
    ref["status"] = status
    spans = {k: _off(D) for k in names}
    spans["status"] = np.arange(F + 1, dtype=np.int64)
    fill = dict(box_of_det=-1, iou=0.0, center=0.0, size=0.0, total=0.0, accepted=0, status=0)
    return Case("assign_2d", F, dict(dets=dets, bbox2d=bbs, front=fronts), ref, spans, fill, ("status",))


# ---- the calls that project: one camera whose W * H is no multiple of 16 ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def camera():
    cam = dict(PC.general_camera())                   # 333 x 141
    cam["dmin"], cam["dmax"] = 0.0, DMAX
    assert (cam["W"] * cam["H"]) % 16 and (cam["W"] * cam["H"]) % 1024
    return cam


@functools.lru_cache(maxsize=None)
def _clouds():
    cam = camera()
    return [np.ascontiguousarray(PC._filler(cam, n, 9100 + f), np.float32) if n else np.zeros((0, 4), np.float32) for f, n in enumerate(POINTS)]


def _rect_masks(rng, M, H, W):
    m = np.zeros((M, H, W), np.uint8)
    for i in range(M):
        x0, y0 = int(rng.integers(0, W - 8)), int(rng.integers(0, H - 8))
        m[i, y0:y0 + int(rng.integers(8, H)), x0:x0 + int(rng.integers(8, W))] = 1
    return m


@functools.lru_cache(maxsize=None)
def _velo_boxes():
    """per frame BOXES[f] velodyne-frame boxes around parts of the frame's own points (float64 [B,8,3])"""
    cam = camera()
    out = []
    for f, (p, nb) in enumerate(zip(_clouds(), BOXES)):
        if nb == 0 or len(p) == 0:
            out.append(np.zeros((0, 8, 3)))
            continue
        out.append(boxes_around(p, nb, 9300 + f))
    return out


def boxes_around(points, nb, seed):
    """nb axis-aligned velodyne-frame boxes (float64 [nb,8,3]) around seeded points of the cloud in front of the camera"""
    rng = np.random.default_rng(seed)
    q = np.asarray(points, np.float64)[:, :3]
    q = q[q[:, 0] > 0.2]
    boxes = []
    for _ in range(nb):
        c = q[int(rng.integers(len(q)))]
        half = rng.uniform(1.0, 6.0, 3)
        boxes.append(PC._aabb(c - half, c + half))
    return np.ascontiguousarray(np.stack(boxes))


@functools.lru_cache(maxsize=None)
def inside_masks(M=3):
    from oracle import numpy_path as npp
    cam, clouds, boxes = camera(), _clouds(), _velo_boxes()
    splits, all_lists = [], []
    for f, (p, c) in enumerate(zip(clouds, boxes)):
        masks = _rect_masks(np.random.default_rng(9400 + f), M, cam["H"], cam["W"])
        lists = npp.frame_path(p, cam["T"], cam["K"], cam["W"], cam["H"], DMAX, masks, c)[3] if len(p) else [np.zeros(0, np.int64)] * M
        splits.append(IR.frame_split(p, lists, c, MIN_POINTS, True))
        all_lists.append([np.asarray(x, np.int64) for x in lists])
    tot = np.array([int(s["off"][-1]) for s in splits])
    cap = int(np.sort(tot)[-2])                       # room for every frame but the one with the longest lists
    assert int(np.argmax(tot)) == OVERFLOW_FRAME and tot[OVERFLOW_FRAME] > cap > 0
    inst_idx, inst_off = np.zeros((F, cap), np.int64), np.zeros((F, M + 1), np.int64)
    best_box, best_cnt = np.full((F, M), -1, np.int32), np.zeros((F, M), np.int64)
    fill = dict(inside=9, part_idx=-7, part_xyz=2.5, n_inside=0, matched=0)
    ref = dict(inside=np.full((F, cap), 9, np.uint8), part_idx=np.full((F, cap), -7, np.int64), part_xyz=np.full((F, cap, 3), 2.5, np.float32),
               n_inside=np.zeros((F, M), np.int64), matched=np.zeros((F, M), np.int32))
    for f, s in enumerate(splits):
        n = int(tot[f])
        inst_off[f], best_box[f], best_cnt[f] = s["off"], s["best_box"], s["best_cnt"]
        ref["matched"][f] = s["matched"]
        if n > cap:                                   # the lists did not fit: the rows are left alone, nothing is counted
            continue
        ref["n_inside"][f] = s["n_inside"]
        for k in ("inside", "part_idx", "part_xyz"):
            ref[k][f, :n] = s[k]
        inst_idx[f, :n] = np.concatenate([np.zeros(0, np.int64)] + all_lists[f])
    spans = {k: np.arange(F + 1, dtype=np.int64) for k in ref}
    inputs = dict(frames=clouds, corners=boxes, inst_idx=inst_idx, inst_off=inst_off, best_box=best_box, best_cnt=best_cnt, M=M, cap=cap)
    case = Case("inside_masks", F, inputs, ref, spans, fill, ("n_inside", "matched"))
    case.splits, case.lists = splits, all_lists
    return case


@functools.lru_cache(maxsize=None)
def box_points():
    cam, clouds, boxes = camera(), _clouds(), _velo_boxes()
    off = _off([len(p) for p in clouds])
    Ntot = int(off[-1])
    valid_idx, n_valid, labels = np.zeros(Ntot, np.int64), np.zeros(F, np.int64), np.zeros(Ntot, np.uint32)
    valid, labelled = [], []
    for f, p in enumerate(clouds):
        vi = BP.valid_indices(p, cam["T"], cam["K"], cam["W"], cam["H"], DMAX) if len(p) else np.zeros(0, np.int64)
        lab = np.random.default_rng(9500 + f).random(len(vi)) < 0.4
        a = int(off[f])
        valid_idx[a:a + len(vi)], n_valid[f] = vi, len(vi)
        labels[a:a + len(vi)] = np.where(lab, np.uint32(1) << np.uint32(f % 32), 0).astype(np.uint32)
        valid.append(vi)
        labelled.append(lab)
    r = BP.batch_box_points(clouds, valid, boxes, labelled, True)
    first = np.full(Ntot, -5, np.int32)               # (the restatement fills with -1: the sentinel here is the caller's)
    for f, vi in enumerate(valid):
        a = int(off[f])
        first[a:a + len(vi)] = r["first_box"][a:a + len(vi)]
    ref = dict(box_points=r["box_points"], box_labelled=r["box_labelled"], first_box=first, frame_counts=np.ascontiguousarray(r["frame_counts"], np.int64))
    boff = _off([len(c) for c in boxes])
    spans = dict(box_points=boff, box_labelled=boff, first_box=off, frame_counts=np.arange(F + 1, dtype=np.int64))
    fill = dict(box_points=0, box_labelled=0, first_box=-5, frame_counts=0)
    inputs = dict(frames=clouds, corners=boxes, valid_idx=valid_idx, n_valid=n_valid, label_valid=labels)
    case = Case("box_points", F, inputs, ref, spans, fill, ("frame_counts",))
    case.valid, case.labelled = valid, labelled
    return case


@functools.lru_cache(maxsize=None)
def box_views():
    calib = load_calib()
    K = np.ascontiguousarray(np.asarray(calib["K"], np.float64)[:3, :3])
    W, H = int(calib["width"]), int(calib["height"])
    Tcv = np.linalg.inv(np.asarray(calib["TrVeloToCam"], np.float64).reshape(4, 4))
    counts = [b for _, b in SHAPES]
    box_off = _off(counts).astype(np.int32)
    corners = BV.seeded_boxes(int(box_off[-1]), seed=23)
    r = BV.views(corners, box_off, K, W, H, Tcv)
    ref = {k: np.ascontiguousarray(r[k]) for k in BV.WANT}
    spans = {k: (np.arange(F + 1, dtype=np.int64) if k == "frame_counts" else box_off.astype(np.int64)) for k in ref}
    inputs = dict(corners=corners, box_off=box_off, K=K, W=W, H=H, T_cam_to_velo=Tcv)
    return Case("box_views", F, inputs, ref, spans, {k: 0 for k in ref}, ("frame_counts",))


@functools.lru_cache(maxsize=None)
def first_match(M=3, mh=120, mw=300):
    cam, clouds = camera(), _clouds()
    off = _off([len(p) for p in clouds])
    Ntot = int(off[-1])
    masks = np.stack([_rect_masks(np.random.default_rng(9600 + f), M, mh, mw) for f in range(F)])
    colors = (np.arange(F * M * 3, dtype=np.float64).reshape(F, M, 3) * 0.25 + 1.0) / 255.0      # rows that tell frame and mask apart
    fill = dict(first_mask=-9, car_idx=-7, car_mask=-7, car_xyz=2.5, car_rgb=3.5, bg_idx=-7, bg_xyz=2.5, n_valid=0, n_car=0, n_bg=0, mask_count=0)
    ref = dict(first_mask=np.full(Ntot, -9, np.int32), car_idx=np.full(Ntot, -7, np.int64), car_mask=np.full(Ntot, -7, np.int32),
               car_xyz=np.full((Ntot, 3), 2.5, np.float32), car_rgb=np.full((Ntot, 3), 3.5, np.float64), bg_idx=np.full(Ntot, -7, np.int64),
               bg_xyz=np.full((Ntot, 3), 2.5, np.float32), n_valid=np.zeros(F, np.int64), n_car=np.zeros(F, np.int64), n_bg=np.zeros(F, np.int64),
               mask_count=np.zeros((F, M), np.int64))
    per = []
    for f, p in enumerate(clouds):
        u, v, valid = FM.project(p, cam["T"], cam["K"], cam["W"], cam["H"], DMAX) if len(p) else (np.zeros(0, int),) * 2 + (np.zeros(0, bool),)
        r = FM.first_match(u, v, valid, masks[f])
        per.append(r)
        a, nc, nb = int(off[f]), len(r["car_idx"]), len(r["bg_idx"])
        ref["first_mask"][a:a + len(p)] = r["first_mask"]
        ref["car_idx"][a:a + nc], ref["car_mask"][a:a + nc] = r["car_idx"], r["car_mask"]
        ref["car_xyz"][a:a + nc], ref["car_rgb"][a:a + nc] = p[r["car_idx"], :3], colors[f][r["car_mask"]]
        ref["bg_idx"][a:a + nb], ref["bg_xyz"][a:a + nb] = r["bg_idx"], p[r["bg_idx"], :3]
        ref["n_valid"][f], ref["n_car"][f], ref["n_bg"][f], ref["mask_count"][f] = nc + nb, nc, nb, r["mask_count"]
    per_frame = ("n_valid", "n_car", "n_bg", "mask_count")
    spans = {k: (np.arange(F + 1, dtype=np.int64) if k in per_frame else off) for k in ref}
    case = Case("first_match", F, dict(frames=clouds, masks=masks, colors=colors), ref, spans, fill, per_frame)
    case.per = per
    return case


FD = 12                                               # frames of the depth-map and overlay cases
MD = 3                                                # cars per frame: 36 images, so that cuts of 5 and 35 fall inside a frame


def depth_image(points, cam):
    """(D float64 [H,W], winner int64 [H,W]) of the definition: the last valid point of a pixel writes its depth (0 / -1: none)"""
    D, win = np.zeros((cam["H"], cam["W"])), np.full((cam["H"], cam["W"]), -1, np.int64)
    if len(points):
        ph = points.copy()
        ph[:, 3] = 1
        pc = np.matmul(cam["T"], ph.T).T[:, :3]
        from oracle import numpy_path as npp
        u, v, depth = npp.cam2image(cam["K"], pc.T)
        ok = np.flatnonzero((u >= 0) & (u < cam["W"]) & (v >= 0) & (v < cam["H"]) & (depth > 0) & (depth < cam["dmax"]))
        D[v[ok], u[ok]] = depth[ok]                   # (ascending point order: the last writer stays)
        win[v[ok], u[ok]] = ok
    return D, win


@functools.lru_cache(maxsize=None)
def depth_maps():
    cam = camera()
    clouds = _clouds()[:FD - 1] + [np.zeros((0, 4), np.float32)]
    H, W = cam["H"], cam["W"]
    masks = np.stack([_rect_masks(np.random.default_rng(9700 + f), MD, H, W) for f in range(FD)])
    masks[5, 1] = 0                                   # an empty car between two others
    maps, car_len = [], np.zeros((FD, MD), np.int64)
    for f, p in enumerate(clouds):
        D, win = depth_image(p, cam)
        cars = []
        for m in range(MD):
            pix = np.flatnonzero(np.where(masks[f, m] > 0, D, 0.0))
            cars.append((pix.astype(np.int64), D.ravel()[pix], win.ravel()[pix].astype(np.int64)))
            car_len[f, m] = len(pix)
        maps.append(cars)
    ref = flat_maps(maps)
    per_frame = _off(car_len.sum(axis=1))
    spans = dict(pix=per_frame, depth=per_frame, point_idx=per_frame, car_len=np.arange(FD + 1, dtype=np.int64))
    case = Case("depth_maps", FD, dict(frames=clouds, masks=masks), ref, spans, dict(pix=0, depth=0.0, point_idx=0, car_len=0), ("car_len",))
    case.maps = maps
    return case


def flat_maps(maps):
    """LpfContext.depth_maps' per-frame car tuples as four arrays: the cars' pixels, depths and winning points one after another, and
    car_len int64 [F, M]"""
    cars = [c for fr in maps for c in fr]
    return dict(pix=_cat([c[0] for c in cars], np.int64), depth=_cat([c[1] for c in cars], np.float64),
                point_idx=_cat([c[2] for c in cars], np.int64),
                car_len=np.array([[len(c[0]) for c in fr] for fr in maps], np.int64).reshape(len(maps), -1))


@functools.lru_cache(maxsize=None)
def depth_overlays():
    cam = camera()
    H, W = cam["H"], cam["W"]
    maps = depth_maps().maps
    seg = np.stack([np.random.default_rng(9800 + f).integers(0, 256, size=(H, W, 3), dtype=np.uint8) for f in range(FD)])
    lut = OV.jet_lut()
    images, mx = np.zeros((FD * MD, H, W, 3), np.uint8), np.zeros(FD * MD)
    for f in range(FD):
        for m in range(MD):
            images[f * MD + m], mx[f * MD + m] = OV.overlay(seg[f], maps[f][m][0], maps[f][m][1], lut)
    items = np.arange(FD * MD + 1, dtype=np.int64)
    ref = dict(images=images, max_depth=mx)
    case = Case("depth_overlays", FD * MD, dict(maps=maps, seg=seg, M=MD), ref, dict(images=items, max_depth=items), dict(images=0, max_depth=0.0),
                ("max_depth",))
    case.nonempty = depth_maps().ref["car_len"].ravel() > 0      # (an empty car's image is only the frame's reversed segmented image)
    return case


def case(call):
    return globals()[call]()
