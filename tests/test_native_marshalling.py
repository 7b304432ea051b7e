"""What the ctypes binding hands to the library, and how it slices what comes back, without a GPU: a recording stub stands in for
liblpf.so.  Per native call it records the scalar arguments and, per struct, every scalar field, NULL-or-not of every pointer field and
a hash of the bytes behind each input pointer; through each output pointer it writes a ramp (or the values a case gives), so the
per-frame slicing of the returned lists and dicts shows in the result.  The record and the result of every case are held against the
literals of EXPECT (below the tests; arrays of more than 12 elements as a hash): the binding may be rearranged, what it marshals may
not move.  (Host arrays only: the GPU-tensor
branches need a GPU and are covered by tests/test_gpu_*.py.)"""
import collections
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from lidar_object_detection_amd import _native as N
from test_wide_api import _NoGpu

H, W = 48, 64


@pytest.fixture(autouse=True)
def _host_arrays_only(monkeypatch):
    """Where torch sees a GPU the binding stages a multi-frame batch of host arrays through a GPU tensor (LpfContext._stage_points) and
    hands the library a device address, which the stub cannot hash from the host: these tests are about host arrays, on every
    machine."""
    try:
        import torch
    except ImportError:
        return
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


# element type of what every pointer field addresses (lpf_outputs.summary: one lpf_frame_summary per frame)
DT = {
    "Outputs": dict(uv="i4", label_bits="u4", depth="f8", u_f="f8", v_f="f8", valid_idx="i8", inst_idx="i8", count_mb="i4",
                    summary=N.SUMMARY_DTYPE, uv_valid="i4", label_valid="u4"),
    "WideInput": dict(masks="u1", rects="i4"),
    "WideOutputs": dict(uv="i4", depth="f8", u_f="f8", v_f="f8", valid_idx="i8", uv_valid="i4", label_words="u4", label_valid_words="u4",
                        inst_idx="i8", count_mb="i4", n_valid="i8", n_labelled="i8", inst_count="i8", inst_off="i8", best_cnt="i8",
                        best_box="i4", inst_overflow="i4"),
    "DepthMapsOutputs": dict(pix="i8", depth="f8", point_idx="i8", car_off="i8", need="i8", overflow="i4"),
    "DepthOverlayInput": dict(pix="i8", depth="f8", car_off="i8", seg="u1"),
    "DepthOverlayOutputs": dict(images="u1", max_depth="f8"),
    "Match2dInput": dict(dets="f4", det_off="i4", bbox2d="f8", front="i4", box_off="i4"),
    "Match2dOutputs": dict(best_box="i4", best_iou="f8", iou="f8", center_score="f8", size_score="f8", total_score="f8", cost="f8"),
    "AssignInput": dict(cost="f8", front="i4", det_off="i4", box_off="i4"),
    "AssignOutputs": dict(col_of_row="i4", status="i4"),
    "Assign2dOutputs": dict(box_of_det="i4", iou="f8", center_score="f8", size_score="f8", total_score="f8", accepted="i4", status="i4"),
    "InsideInput": dict(inst_idx="i8", inst_off="i8", best_box="i4", best_cnt="i8"),
    "InsideOutputs": dict(inside="u1", part_idx="i8", part_xyz="f4", n_inside="i8", matched="i4"),
    "BoxPointsInput": dict(valid_idx="i8", n_valid="i8", label_valid_words="u4"),
    "BoxPointsOutputs": dict(box_points="i4", box_labelled="i4", first_box="i4", frame_counts="i8"),
    "BoxViewsInput": dict(corners_cam0="f8", box_off="i4", T_cam_to_velo="f8"),
    "BoxViewsOutputs": dict(keep="u1", reason="i4", corners_in_view="i4", corners_near="i4", avg_depth="f8", near_bbox2d="f8", front="i4",
                            bbox2d="f8", front_avg_depth="f8", kept_pos="i4", frame_counts="i4", corners_velo="f8"),
    "CamInput": dict(corners_velo="f8", box_off="i4"),
}
WITH_POINTS = ("lpf_run_batch", "lpf_run_wide", "lpf_depth_maps", "lpf_inside_masks", "lpf_box_points", "lpf_run_cams", "lpf_run_cams_wide")


def _sha(b):
    return hashlib.sha1(bytes(b)).hexdigest()[:12]


def _at(addr, dtype, n):
    dtype = np.dtype(dtype)
    return np.frombuffer((ctypes.c_uint8 * (n * dtype.itemsize)).from_address(addr), dtype=dtype)


class Stub:
    """Stands in for ctx._lib.  counts: per pointer field the elements behind it (a number, or a function of the struct); a pointer
    without a count is recorded as NULL or not only.  writes: per call of a function (the last entry repeats) the values to put behind
    output pointers in place of the ramp.  filled: output fields whose bytes the binding sets before the call -- they are recorded."""

    def __init__(self, counts, writes=({},), filled=()):
        self.counts, self.writes, self.filled = counts, writes, filled
        self.calls, self.bufs, self.seen = [], [], collections.Counter()

    def lpf_host_alloc(self, nbytes):
        self.bufs.append((ctypes.c_uint8 * nbytes)())           # kept alive: the context frees through lpf_host_free, a no-op here
        return ctypes.addressof(self.bufs[-1])

    def lpf_host_free(self, p):
        pass

    def lpf_last_error(self, h):
        return None

    def __getattr__(self, name):
        if not name.startswith("lpf_"):
            raise AttributeError(name)
        return functools.partial(self._call, name)

    def _call(self, name, h, *args):
        writes = self.writes[min(self.seen[name], len(self.writes) - 1)]
        self.seen[name] += 1
        rec = [name]
        if name in WITH_POINTS:
            pts, off, F, dev = args[:4]
            args = args[4:]
            off = _at(off, "i8", F + 1)
            rec += [F, dev, off.tolist(), "NULL" if pts is None else _sha(_at(pts, "f4", 4 * int(off[-1])))]
        for a in args:
            if isinstance(a, (int, float)):
                rec.append(a)
            else:
                structs = list(a) if isinstance(a, ctypes.Array) else [a._obj]
                rec.append([self._struct(s, k, "", writes) for k, s in enumerate(structs)])
        self.calls.append(rec)
        return 0

    def _struct(self, s, k, prefix, writes):
        cls, rec = type(s).__name__, {}
        is_out = cls.endswith("Outputs")
        for i, (f, t) in enumerate(s._fields_):
            v = getattr(s, f)
            if isinstance(v, ctypes.Structure):
                rec[f] = self._struct(v, k, f + ".", writes)
            elif isinstance(v, ctypes.Array):
                rec[f] = list(v)
            elif t is not ctypes.c_void_p:
                rec[f] = v
            elif v is None:
                rec[f] = "NULL"
            elif prefix + f not in self.counts:
                rec[f] = "ptr"
            else:
                n = self.counts[prefix + f]
                mem = _at(v, DT[cls][f], n(s) if callable(n) else n)
                if not is_out:
                    rec[f] = "in[%d] %s" % (len(mem), _sha(mem))
                    continue
                rec[f] = "out[%d]" % len(mem)
                if f in self.filled:                        # what the binding put there: one value throughout, or a hash
                    was = np.unique(mem.view(np.uint8) if mem.dtype.names else mem)
                    rec[f] += " was all %s" % was[0] if len(was) == 1 else " was " + _sha(mem)
                mem[:] = writes[f] if f in writes else (np.arange(len(mem)) + 7 * i + 1000 * k).astype(mem.dtype)
        return rec


class Ctx(_NoGpu):
    """_NoGpu with the state LpfContext.__init__ leaves behind and a Stub for the library"""
    def __init__(self, stub, M=0, F_masks=0, box_off=None):
        super().__init__()
        self._lib, self._h, self._pin, self._lent = stub, None, {}, collections.deque(maxlen=4)
        self.device, self.M, self.F_masks = 0, M, F_masks
        self.box_off = None if box_off is None else np.asarray(box_off, np.int32)


def _canon(x):
    if isinstance(x, dict):
        return {str(k): _canon(v) for k, v in x.items()}                 # (in the dict's own order: it is part of what is returned)
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    if isinstance(x, np.ndarray):
        return "%s%s %s" % (x.dtype.str, list(x.shape), x.tolist() if x.size <= 12 else _sha(np.ascontiguousarray(x)))
    if isinstance(x, np.generic):
        return x.item()
    return x


def _frames(F, empty=False):
    """F = 1: six points; F = 2: six and four; empty: one frame without a point"""
    sizes = [0] if empty else [6, 4][:F]
    return [((np.arange(4 * n) * (f + 3)) % 11).astype(np.float32).reshape(n, 4) for f, n in enumerate(sizes)]


# ---- the run paths --------------------------------------------------------------------------------------------------------------------
BOX_OFF = {1: [0, 3], 2: [0, 2, 3]}


def _summary(F, overflow=0):
    s = np.zeros(F, N.SUMMARY_DTYPE)
    for f in range(F):
        s[f]["n_valid"], s[f]["n_labelled"] = 4 - f, 2 - f
        s[f]["inst_count"][:2], s[f]["inst_off"][:3] = (2 - f, 1 + f), (0, 2 - f, 3)
        s[f]["best_cnt"][:2], s[f]["best_box"][:2] = (5, 6 + f), (1, -1)
        s[f]["inst_overflow"], s[f]["inst_off"][32] = overflow, 9
    return s


def _run_counts(F, n, M, Btot):
    return dict(uv=2 * n, label_bits=n, depth=n, u_f=n, v_f=n, valid_idx=n, uv_valid=2 * n, label_valid=n,
                inst_idx=lambda o: F * o.inst_cap, count_mb=max(M * Btot, 1), summary=F)


RUN_FILLED = ("count_mb", "summary")
ALL_ON = dict(want_uv=True, want_label=True, want_float=True, want_lists=True, want_valid_uv=True)


def _run_batch(F=2, overflow=False, **kw):
    n = 10 if F == 2 else 6
    writes = [dict(summary=_summary(F, 1)), dict(summary=_summary(F))] if overflow else [dict(summary=_summary(F))]
    stub = Stub(_run_counts(F, n, 2, 3), writes, RUN_FILLED)
    res = Ctx(stub, M=2, F_masks=F, box_off=BOX_OFF[F]).run_batch(_frames(F), **kw)
    return stub, res


def _wide_writes(F, M, overflow=0):
    io = np.zeros((F, M + 1), np.int64)
    if M:
        io[:, 1:] = [[2 - f, 3] for f in range(F)]
    return dict(n_valid=np.arange(4, 4 - F, -1), inst_off=io.reshape(-1), inst_overflow=np.full(F, overflow))


def _wide_counts(F, n, M, Btot):
    LW = (M + 31) // 32
    return dict(uv=2 * n, depth=n, u_f=n, v_f=n, valid_idx=n, uv_valid=2 * n, label_words=n * LW, label_valid_words=n * LW,
                inst_idx=lambda o: F * o.inst_cap, count_mb=max(M * Btot, 1), n_valid=F, n_labelled=F, inst_count=F * M,
                inst_off=F * (M + 1), best_cnt=F * M, best_box=F * M, inst_overflow=F, masks=F * M * H * W, rects=F * M * 4)


WIDE_FILLED = ("count_mb", "n_valid", "n_labelled", "inst_count", "inst_off", "best_cnt", "best_box", "inst_overflow")


def _masks(F, M):
    return ((np.arange(F * M * H * W) % 5) == 0).astype(np.uint8).reshape(F, M, H, W)


def _rects(F, M):
    return (np.arange(F * M * 4) % 9).astype(np.int32).reshape(F, M, 4)


def _run_wide(F=2, M=2, rects=False, overflow=False, **kw):
    n = 10 if F == 2 else 6
    writes = [_wide_writes(F, M, 1), _wide_writes(F, M)] if overflow else [_wide_writes(F, M)]
    stub = Stub(_wide_counts(F, n, M, 3), writes, WIDE_FILLED)
    res = Ctx(stub, box_off=BOX_OFF[F]).run_wide(_frames(F), _masks(F, M), rects=_rects(F, M) if rects else None, **kw)
    return stub, res


def _cams(F, M, rects, boxes):
    cams = []
    for k in range(2):
        cam = dict(T_velo_to_rect=np.eye(4) + k, K=np.eye(3) * (k + 2), width=W, height=H, masks=_masks(F, M) if M else None,
                   erode_iters=k, depth_max=40.0 + k)
        if rects and M:
            cam["rects"] = _rects(F, M) + k
        if boxes:
            cam["boxes"] = [np.arange(24.0 * b).reshape(b, 8, 3) + k for b in np.diff(BOX_OFF[F])]
            cam["oriented"] = not k
        cams.append(cam)
    return cams


def _run_cams(wide, F=2, M=2, rects=False, boxes=True, **kw):
    n = 10 if F == 2 else 6
    Btot = 3 if boxes else 0
    counts = dict(_wide_counts(F, n, M, Btot) if wide else _run_counts(F, n, M, Btot), corners_velo=Btot * 24, box_off=F + 1)
    counts.update({"masks.masks": F * M * H * W, "masks.rects": F * M * 4})
    stub = Stub(counts, [_wide_writes(F, M) if wide else dict(summary=_summary(F))], WIDE_FILLED if wide else RUN_FILLED)
    ctx = Ctx(stub)
    res = (ctx.run_cams_wide if wide else ctx.run_cams)(_frames(F), _cams(F, M, rects, boxes), **kw)
    return stub, res


# ---- the analysis calls ---------------------------------------------------------------------------------------------------------------
def _depth_maps(F=2, M=2, overflow=False, **kw):
    car_off = np.array([[0, 1, 3], [0, 2, 2]][:F], np.int64)[:, :M + 1].reshape(-1)
    first = dict(car_off=car_off, need=np.array([3, 7][:F]), overflow=np.array([0, 1][:F]))
    writes = [first, dict(first, overflow=np.zeros(F, np.int32))] if overflow else [dict(first, overflow=np.zeros(F, np.int32))]
    per_cap = lambda o: F * o.cap
    stub = Stub(dict(pix=per_cap, depth=per_cap, point_idx=per_cap, car_off=F * (M + 1), need=F, overflow=F, masks=F * M * H * W,
                     rects=F * M * 4), writes, ("car_off", "need", "overflow"))
    res = Ctx(stub).depth_maps(_frames(F), _masks(F, M), **kw)
    return stub, res


def _depth_overlays(F=2, M=2):
    maps = [[(np.array([3, 5 + m, 40 + f]), np.array([1.5, 2.0 + f, 0.25 * (m + 1)]), None) for m in range(M)] for f in range(F)]
    if F and M:
        maps[0][0] = (np.zeros(0, np.int64), np.zeros(0, np.float64), None)           # an empty car
    seg = (np.arange(F * H * W * 3) % 251).astype(np.uint8).reshape(F, H, W, 3)
    per_cap = lambda s: F * s.cap
    stub = Stub(dict(pix=per_cap, depth=per_cap, car_off=F * (M + 1), seg=F * H * W * 3, images=F * M * H * W * 3, max_depth=F * M), filled=("max_depth",))
    res = Ctx(stub).depth_overlays(maps, seg)
    return stub, res


def _match_2d(D=(2, 1), B=(2, 1), dtype=np.float32, **kw):
    F = len(D)
    dets = [(np.arange(4 * d) + f).astype(dtype).reshape(d, 4) for f, d in enumerate(D)]
    bbox2d = [np.arange(4.0 * b).reshape(b, 4) * (f + 1) for f, b in enumerate(B)]
    front = [np.arange(b, dtype=np.int32) + f for f, b in enumerate(B)]
    Dtot, Btot, P = sum(D), sum(B), sum(d * b for d, b in zip(D, B))
    stub = Stub(dict(dets=Dtot * (2 if dtype == np.float64 else 1) * 4, det_off=F + 1, bbox2d=Btot * 4, front=Btot, box_off=F + 1, best_box=Dtot,
                     best_iou=Dtot, iou=P, center_score=P, size_score=P, total_score=P, cost=P), filled=("best_box", "best_iou"))
    res = Ctx(stub).match_2d(dets, bbox2d, front, **kw)
    return stub, res


def _assign_costs(shapes=((2, 3), (3, 1)), front=False, status=None, **kw):
    """status: what the library reports per frame (zeros: every frame solved; the ramp would be an error).  Every third row is unassigned."""
    F = len(shapes)
    costs = [((np.arange(d * b) * (f + 2)) % 7).astype(np.float64).reshape(d, b) for f, (d, b) in enumerate(shapes)]
    fronts = [(np.arange(b, dtype=np.int32) + f) % 3 for f, (d, b) in enumerate(shapes)] if front else None
    Dtot, Btot, P = sum(d for d, _ in shapes), sum(b for _, b in shapes), sum(d * b for d, b in shapes)
    writes = dict(col_of_row=np.arange(Dtot) % 3 - 1, status=np.zeros(F, np.int32) if status is None else np.asarray(status, np.int32))
    stub = Stub(dict(cost=P, front=Btot, det_off=F + 1, box_off=F + 1, col_of_row=Dtot, status=F), [writes], ("col_of_row", "status"))
    try:
        res = Ctx(stub).assign_costs(costs, fronts, **kw)
    except ValueError as e:
        res = "ValueError: %s" % e
    return stub, res


def _assign_2d(D=(2, 1), B=(2, 1), dtype=np.float32, **kw):
    F = len(D)
    dets = [(np.arange(4 * d) + f).astype(dtype).reshape(d, 4) for f, d in enumerate(D)]
    bbox2d = [np.arange(4.0 * b).reshape(b, 4) * (f + 1) for f, b in enumerate(B)]
    front = [np.arange(b, dtype=np.int32) + f for f, b in enumerate(B)]
    Dtot, Btot = sum(D), sum(B)
    stub = Stub(dict(dets=Dtot * (2 if dtype == np.float64 else 1) * 4, det_off=F + 1, bbox2d=Btot * 4, front=Btot, box_off=F + 1, box_of_det=Dtot,
                     iou=Dtot, center_score=Dtot, size_score=Dtot, total_score=Dtot, accepted=Dtot, status=F), filled=tuple(DT["Assign2dOutputs"]))
    res = Ctx(stub).assign_2d(dets, bbox2d, front, **kw)
    return stub, res


INSIDE_DT = dict(inside=np.uint8, part_idx=np.int64, part_xyz=np.float32, n_inside=np.int64, matched=np.int32)


def _inside(F=2, M=2, cap=5, want=N.LpfContext.INSIDE_WANT, out=False, staged=False, **kw):
    n = 10 if F == 2 else 6
    idx = (np.arange(F * cap) % 4).reshape(F, cap)
    off = np.array([[0, 2, 5], [0, 1, 3]][:F])
    box, cnt = np.array([[1, -1], [0, 2]][:F], np.int32), np.array([[12, 0], [3, 30]][:F])
    shape = dict(inside=(F, cap), part_idx=(F, cap), part_xyz=(F, cap, 3), n_inside=(F, M), matched=(F, M))
    stub = Stub(dict(inst_idx=F * cap, inst_off=F * (M + 1), best_box=F * M, best_cnt=F * M, inside=F * cap, part_idx=F * cap,
                     part_xyz=F * cap * 3, n_inside=F * M, matched=F * M), filled=N.LpfContext.INSIDE_WANT)
    ctx = Ctx(stub, box_off=BOX_OFF[F])
    if out:
        kw["out"] = {w: np.full(shape[w], 5, INSIDE_DT[w]) for w in want[:2]}
    if staged:
        kw["staged"] = ctx.stage_points(_frames(F))
    res = ctx.inside_masks(None if staged else _frames(F), idx, off, box, cnt, want=want, **kw)
    assert set(res) == set(want) and all(res[w] is a for w, a in kw.get("out", {}).items())
    assert all(res[w].shape == shape[w] and res[w].dtype == INSIDE_DT[w] for w in want)
    return stub, res


BP_DT = dict(box_points=np.int32, box_labelled=np.int32, first_box=np.int32, frame_counts=np.int64)


def _box_points(F=2, label=None, want=N.LpfContext.BOX_POINTS_WANT, out=False, staged=False, empty=False, **kw):
    frames = _frames(F, empty)
    n = sum(len(p) for p in frames)
    vi, nv = np.arange(n)[::-1].copy(), np.array([4, 3][:F])
    lv = None if label is None else (np.arange(n * label) % 3).astype(np.uint32).reshape((n,) if label == 1 else (n, label))
    if label == 1 and kw.pop("flat", True) is False:
        lv = lv.reshape(n, 1)
    shape = dict(box_points=(3,), box_labelled=(3,), first_box=(n,), frame_counts=(F, 4))
    stub = Stub(dict(valid_idx=max(n, 1), n_valid=F, label_valid_words=n * (label or 0), box_points=3, box_labelled=3, first_box=n,
                     frame_counts=F * 4), filled=N.LpfContext.BOX_POINTS_WANT)
    ctx = Ctx(stub, box_off=BOX_OFF[F])
    if out:
        kw["out"] = {w: np.full(shape[w], 5, BP_DT[w]) for w in want[:2]}
    if staged:
        kw["staged"] = ctx.stage_points(frames)
    res = ctx.box_points(None if staged else frames, vi, nv, lv, want=want, **kw)
    assert set(res) == set(want) and all(res[w] is a for w, a in kw.get("out", {}).items())
    assert all(res[w].shape == shape[w] and res[w].dtype == BP_DT[w] for w in want)
    return stub, res


def _box_views(T=False, **kw):
    corners = np.arange(3 * 24.0).reshape(3, 8, 3) / 7
    stub = Stub(dict(corners_cam0=72, box_off=3, T_cam_to_velo=16, keep=3, reason=3, corners_in_view=3, corners_near=3, avg_depth=3,
                     near_bbox2d=12, front=3, bbox2d=12, front_avg_depth=3, kept_pos=3, frame_counts=12, corners_velo=72),
                filled=N.LpfContext.BOX_VIEWS_WANT)
    if T:
        kw["T_cam_to_velo"] = np.arange(16.0).reshape(4, 4)
    res = Ctx(stub).box_views(corners, [0, 2, 3], **kw)
    return stub, res


P = functools.partial
CASES = {
    "run_batch": P(_run_batch),
    "run_batch F=1": P(_run_batch, F=1),
    "run_batch all on": P(_run_batch, **ALL_ON),
    **{"run_batch %s off" % k: P(_run_batch, **dict(ALL_ON, **{k: False})) for k in ALL_ON},
    "run_batch pinned": P(_run_batch, pinned=True, **ALL_ON),
    "run_batch lists did not fit": P(_run_batch, overflow=True),
    "run_batch inst_cap": P(_run_batch, inst_cap=3),
    "run_wide M=0": P(_run_wide, M=0),
    "run_wide M=2": P(_run_wide),
    "run_wide M=2 F=1 rects": P(_run_wide, F=1, rects=True, binarize="gt0.5", erode_iters=2),
    "run_wide all on": P(_run_wide, rects=True, want_float=True, want_valid_uv=True),
    "run_wide no uv no lists": P(_run_wide, want_uv=False, want_lists=False),
    "run_wide lists did not fit": P(_run_wide, overflow=True),
    "run_cams M=0": P(_run_cams, False, M=0),
    "run_cams M=2": P(_run_cams, False),
    "run_cams M=2 rects no boxes": P(_run_cams, False, rects=True, boxes=False, **ALL_ON),
    "run_cams pinned": P(_run_cams, False, F=1, pinned=True, **ALL_ON),
    "run_cams_wide M=0": P(_run_cams, True, M=0),
    "run_cams_wide M=2": P(_run_cams, True),
    "run_cams_wide M=2 rects no boxes": P(_run_cams, True, rects=True, boxes=False, want_float=True, want_valid_uv=True),
    "run_cams_wide pinned no label": P(_run_cams, True, F=1, pinned=True, want_label=False, want_valid_uv=True),
    "depth_maps": P(_depth_maps, cap=4),
    "depth_maps default cap F=1": P(_depth_maps, F=1),
    "depth_maps M=0": P(_depth_maps, M=0),
    "depth_maps overflow": P(_depth_maps, cap=4, overflow=True, want_point_idx=False, rects=_rects(2, 2), erode_iters=1),
    "depth_overlays": P(_depth_overlays),
    "depth_overlays F=1": P(_depth_overlays, F=1),
    "depth_overlays M=0": P(_depth_overlays, M=0),
    "match_2d best": P(_match_2d),
    "match_2d one matrix": P(_match_2d, want=("center",)),
    "match_2d everything": P(_match_2d, dtype=np.float64, want=N.LpfContext.MATCH2D_WANT, min_iou=0.5, weights=(0.25, 0.5, 0.125)),
    "match_2d F=1": P(_match_2d, D=(2,), B=(3,), want=("best", "cost")),
    "match_2d no detections": P(_match_2d, D=(0, 0), want=("best", "iou")),
    "match_2d no boxes": P(_match_2d, B=(0, 0), want=("best", "iou")),
    "assign_costs": P(_assign_costs),
    "assign_costs front": P(_assign_costs, front=True),
    "assign_costs raw": P(_assign_costs, raw=True),
    "assign_costs F=1": P(_assign_costs, shapes=((2, 3),)),
    "assign_costs no rows, no columns": P(_assign_costs, shapes=((0, 3), (2, 0)), front=True),
    "assign_costs a frame without an assignment": P(_assign_costs, status=(0, 2)),
    "assign_2d": P(_assign_2d),
    "assign_2d float64": P(_assign_2d, dtype=np.float64, weights=(0.25, 0.5, 0.125), min_score_threshold=0.5, min_iou_threshold=0.125),
    "assign_2d two outputs": P(_assign_2d, want=("box_of_det", "status")),
    "assign_2d F=1": P(_assign_2d, D=(2,), B=(3,)),
    "assign_2d no detections": P(_assign_2d, D=(0, 0)),
    "assign_2d no boxes": P(_assign_2d, B=(0, 0)),
    **{"inside_masks %s" % w: P(_inside, want=(w,)) for w in N.LpfContext.INSIDE_WANT},
    "inside_masks all": P(_inside, min_points=3),
    "inside_masks F=1": P(_inside, F=1),
    "inside_masks out": P(_inside, out=True),
    "inside_masks staged": P(_inside, staged=True),
    **{"box_points %s" % w: P(_box_points, want=(w,)) for w in N.LpfContext.BOX_POINTS_WANT},
    "box_points all": P(_box_points),
    "box_points out": P(_box_points, out=True, F=1),
    "box_points staged": P(_box_points, staged=True),
    "box_points label [N]": P(_box_points, label=1),
    "box_points label [N,1]": P(_box_points, label=1, flat=False),
    "box_points label [N,2]": P(_box_points, label=2),
    "box_points Ntot=0": P(_box_points, F=1, empty=True, label=1),
    "box_views": P(_box_views),
    "box_views T": P(_box_views, T=True, want=N.LpfContext.BOX_VIEWS_WANT, min_points_in_view=2, depth_range=(0.5, 80), min_area=50),
    "box_views frame_counts": P(_box_views, want=("frame_counts",)),
}

def record(case):
    """[the native calls as the stub saw them, what the binding returned], in plain lists, dicts, numbers and strings"""
    stub, res = CASES[case]()                # (the stub owns the page-locked buffers that pinned results are views of)
    return _canon([stub.calls, res])


@pytest.mark.parametrize("case", list(CASES))
def test_marshalling_is_what_it_was(case):
    assert record(case) == EXPECT[case]


def test_slicing_of_a_run():
    """the ramp behind the pointers comes back cut at the frames' offsets, n_valid and the instance offsets"""
    stub, (r0, r1) = _run_batch(**ALL_ON)
    calls = stub.calls
    assert len(calls) == 1 and calls[0][1:4] == [2, 0, [0, 6, 10]]
    assert r0["u"].tolist() == [0, 2, 4, 6, 8, 10] and r1["v"].tolist() == [13, 15, 17, 19]              # uv: field 0, [n, 2]
    assert r1["label_bits"].tolist() == [13, 14, 15, 16] and r0["valid_idx"].tolist() == [35, 36, 37, 38]
    assert r1["valid_idx"].tolist() == [41, 42, 43] and r1["u_valid"].tolist() == [96, 98, 100]
    assert [a.tolist() for a in r0["inst_lists"]] == [[42, 43], [44]] and [a.tolist() for a in r1["inst_lists"]] == [[48], [49, 50]]
    assert r0["count_mb"].tolist() == [[56, 57], [58, 59]] and r1["count_mb"].tolist() == [[60], [61]]
    assert r1["n_valid"] == 3 and r0["best_box"].tolist() == [1, -1] and r1["best_cnt"].tolist() == [5, 7]


def test_slicing_of_the_analysis_calls():
    stub, res = _match_2d(want=("best", "cost"))
    o = stub.calls[0][3][0]
    assert o["best_box"].startswith("out[3] was ") and o["iou"] == "NULL" and o["cost"].startswith("out[5]")
    assert [a.tolist() for a in res["best_box"]] == [[0, 1], [2]] and [a.tolist() for a in res["cost"]] == [[[42, 43], [44, 45]], [[46]]]
    stub, res = _assign_2d()                                   # per-frame cuts of the ramp at det_off; status comes back whole
    assert [a.tolist() for a in res["box_of_det"]] == [[0, 1], [2]] and [a.tolist() for a in res["total"]] == [[28, 29], [30]]
    assert [a.tolist() for a in res["accepted"]] == [[35, 36], [37]] and res["status"].tolist() == [42, 43]
    stub, raw = _assign_costs(raw=True, status=(0, 1))
    assert raw["col_of_row"].tolist() == [-1, 0, 1, -1, 0] and raw["status"].tolist() == [0, 1]
    stub, pairs = _assign_costs()                            # rows 0 .. 1 and 2 .. 4 of col_of_row, the rows without a column left out
    assert [[a.tolist() for a in fr] for fr in pairs] == [[[1], [0]], [[0, 2], [1, 0]]]
    stub, maps = _depth_maps(cap=4, overflow=True)
    assert [c[6][0]["cap"] for c in stub.calls] == [4, 7]                  # the second launch asks for what the first one needed
    assert [[c[0].tolist() for c in fr] for fr in maps] == [[[0], [1, 2]], [[7, 8], []]]
    stub, (images, mx) = _depth_overlays()
    assert images.shape == (2, 2, H, W, 3) and images[1, 0, 0, 0].tolist() == [0, 1, 2] and mx.tolist() == [[7, 8], [9, 10]]


EXPECT = {
    'run_batch':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[12]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch F=1':
        [[['lpf_run_batch', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'uv': 'out[12]', 'label_bits': 'out[6]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[6]', 'inst_idx': 'out[6]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[1] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'],
           'count_mb': '<i8[2, 3] [[56, 57, 58], [59, 60, 61]]'}]],
    'run_batch all on':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
           'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'valid_idx': '<i8[4] [35, 36, 37, 38]',
           'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]', 'u_valid': '<i4[4] [84, 86, 88, 90]',
           'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'],
           'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]', 'u_valid': '<i4[3] [96, 98, 100]',
           'v_valid': '<i4[3] [97, 99, 101]', 'label_valid': '<u4[3] [97, 98, 99]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'],
           'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch want_uv off':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'NULL', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]', 'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]',
           'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]', 'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]',
           'u_valid': '<i4[4] [84, 86, 88, 90]', 'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]',
           'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'label_bits': '<u4[4] [13, 14, 15, 16]', 'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]',
           'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]', 'valid_idx': '<i8[3] [41, 42, 43]', 'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]',
           'u_valid': '<i4[3] [96, 98, 100]', 'v_valid': '<i4[3] [97, 99, 101]', 'label_valid': '<u4[3] [97, 98, 99]',
           'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch want_label off':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'NULL', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]',
           'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]', 'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]',
           'u_valid': '<i4[4] [84, 86, 88, 90]', 'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]',
           'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]',
           'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]', 'valid_idx': '<i8[3] [41, 42, 43]',
           'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]', 'u_valid': '<i4[3] [96, 98, 100]', 'v_valid': '<i4[3] [97, 99, 101]',
           'label_valid': '<u4[3] [97, 98, 99]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch want_float off':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[12]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'out[20]',
             'label_valid': 'out[10]'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]',
           'u_valid': '<i4[4] [84, 86, 88, 90]', 'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]',
           'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]', 'u_valid': '<i4[3] [96, 98, 100]',
           'v_valid': '<i4[3] [97, 99, 101]', 'label_valid': '<u4[3] [97, 98, 99]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'],
           'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch want_lists off':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'NULL',
             'inst_idx': 'NULL', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'NULL', 'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
           'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]',
           'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch want_valid_uv off':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'NULL', 'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
           'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'valid_idx': '<i8[4] [35, 36, 37, 38]',
           'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch pinned':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
           'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'valid_idx': '<i8[4] [35, 36, 37, 38]',
           'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]', 'u_valid': '<i4[4] [84, 86, 88, 90]',
           'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'],
           'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]', 'u_valid': '<i4[3] [96, 98, 100]',
           'v_valid': '<i4[3] [97, 99, 101]', 'label_valid': '<u4[3] [97, 98, 99]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'],
           'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch lists did not fit':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[12]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]],
          ['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[18]',
             'inst_cap': 9, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': ['<i8[1] [51]', '<i8[2] [52, 53]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_batch inst_cap':
        [[['lpf_run_batch', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[6]',
             'inst_cap': 3, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
           'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
           'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
          {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
           'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
           'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': ['<i8[1] [45]', '<i8[2] [46, 47]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}]],
    'run_wide M=0':
        [[['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'NULL',
             'label_valid_words': 'NULL', 'inst_idx': 'NULL', 'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'NULL', 'inst_off': 'out[2] was all 0', 'best_cnt': 'NULL', 'best_box': 'NULL',
             'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
           'label_words': '<u4[6, 0] [[], [], [], [], [], []]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
           'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': [], 'count_mb': '<i8[0, 2] []'},
          {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
           'label_words': '<u4[4, 0] [[], [], [], []]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
           'valid_idx': '<i8[3] [34, 35, 36]', 'inst_lists': [], 'count_mb': '<i8[0, 1] []'}]],
    'run_wide M=2':
        [[['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
           'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
           'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 2] [[70, 71], [72, 73]]'},
          {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
           'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
           'valid_idx': '<i8[3] [34, 35, 36]', 'inst_lists': ['<i8[1] [62]', '<i8[2] [63, 64]'], 'count_mb': '<i8[2, 1] [[74], [75]]'}]],
    'run_wide M=2 F=1 rects':
        [[['lpf_run_wide', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'masks': 'in[6144] c30a70aebf56', 'rects': 'in[8] 643f7c1d25ad', 'M': 2, 'f32': 0, 'binarize': 2, 'erode_iters': 2, 'on_device': 0,
             'reserved': 0}],
           [{'uv': 'out[12]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[6]', 'uv_valid': 'NULL', 'label_words': 'out[6]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[6]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[1] was all 0',
             'n_labelled': 'out[1] was all 0', 'inst_count': 'out[2] was all 0', 'inst_off': 'out[3] was all 0', 'best_cnt': 'out[2] was all 0',
             'best_box': 'out[2] was all -1', 'inst_overflow': 'out[1] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
           'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
           'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'],
           'count_mb': '<i8[2, 3] [[70, 71, 72], [73, 74, 75]]'}]],
    'run_wide all on':
        [[['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] ff5d7a01baa9', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0,
             'reserved': 0}],
           [{'uv': 'out[20]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]', 'uv_valid': 'out[20]',
             'label_words': 'out[10]', 'label_valid_words': 'out[10]', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0',
             'n_valid': 'out[2] was all 0', 'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0',
             'best_cnt': 'out[4] was all 0', 'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
           'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
           'depth': '<f8[6] [7.0, 8.0, 9.0, 10.0, 11.0, 12.0]', 'uf': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]',
           'vf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]', 'valid_idx': '<i8[4] [28, 29, 30, 31]',
           'uv_valid': '<i4[4, 2] [[35, 36], [37, 38], [39, 40], [41, 42]]', 'u_valid': '<i4[4] [35, 37, 39, 41]',
           'v_valid': '<i4[4] [36, 38, 40, 42]', 'label_valid_words': '<u4[4, 1] [[49], [50], [51], [52]]',
           'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 2] [[70, 71], [72, 73]]'},
          {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
           'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
           'depth': '<f8[4] [13.0, 14.0, 15.0, 16.0]', 'uf': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'vf': '<f8[4] [27.0, 28.0, 29.0, 30.0]',
           'valid_idx': '<i8[3] [34, 35, 36]', 'uv_valid': '<i4[3, 2] [[47, 48], [49, 50], [51, 52]]', 'u_valid': '<i4[3] [47, 49, 51]',
           'v_valid': '<i4[3] [48, 50, 52]', 'label_valid_words': '<u4[3, 1] [[55], [56], [57]]', 'inst_lists': ['<i8[1] [62]', '<i8[2] [63, 64]'],
           'count_mb': '<i8[2, 1] [[74], [75]]'}]],
    'run_wide no uv no lists':
        [[['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'uv': 'NULL', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'NULL', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'NULL', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
           'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'count_mb': '<i8[2, 2] [[70, 71], [72, 73]]'},
          {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
           'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'count_mb': '<i8[2, 1] [[74], [75]]'}]],
    'run_wide lists did not fit':
        [[['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]],
          ['lpf_run_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[6]', 'inst_cap': 3, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
           'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
           'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 2] [[70, 71], [72, 73]]'},
          {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
           'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
           'valid_idx': '<i8[3] [34, 35, 36]', 'inst_lists': ['<i8[1] [59]', '<i8[2] [60, 61]'], 'count_mb': '<i8[2, 1] [[74], [75]]'}]],
    'run_cams M=0':
        [[['lpf_run_cams', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0},
             'corners_velo': 'in[72] 6ed0631adb52', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0, 'reserved': 0},
             'corners_velo': 'in[72] d4972ac5f49b', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'NULL',
             'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'},
            {'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'NULL',
             'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [[{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
            'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': [], 'count_mb': '<i8[0, 2] []'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
            'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': [], 'count_mb': '<i8[0, 1] []'}],
          [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'label_bits': '<u4[6] [1007, 1008, 1009, 1010, 1011, 1012]', 'valid_idx': '<i8[4] [1035, 1036, 1037, 1038]', 'inst_lists': [],
            'count_mb': '<i8[0, 2] []'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'u': '<i4[4] [1012, 1014, 1016, 1018]', 'v': '<i4[4] [1013, 1015, 1017, 1019]', 'label_bits': '<u4[4] [1013, 1014, 1015, 1016]',
            'valid_idx': '<i8[3] [1041, 1042, 1043]', 'inst_lists': [], 'count_mb': '<i8[0, 1] []'}]]],
    'run_cams M=2':
        [[['lpf_run_cams', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 6ed0631adb52', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] d4972ac5f49b', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[12]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'},
            {'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'inst_idx': 'out[12]',
             'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0, 'uv_valid': 'NULL',
             'label_valid': 'NULL'}]]],
         [[{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
            'valid_idx': '<i8[4] [35, 36, 37, 38]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'], 'count_mb': '<i8[2, 2] [[56, 57], [58, 59]]'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
            'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
            'valid_idx': '<i8[3] [41, 42, 43]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'], 'count_mb': '<i8[2, 1] [[60], [61]]'}],
          [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'label_bits': '<u4[6] [1007, 1008, 1009, 1010, 1011, 1012]', 'valid_idx': '<i8[4] [1035, 1036, 1037, 1038]',
            'inst_lists': ['<i8[2] [1042, 1043]', '<i8[1] [1044]'], 'count_mb': '<i8[2, 2] [[1056, 1057], [1058, 1059]]'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
            'u': '<i4[4] [1012, 1014, 1016, 1018]', 'v': '<i4[4] [1013, 1015, 1017, 1019]', 'label_bits': '<u4[4] [1013, 1014, 1015, 1016]',
            'valid_idx': '<i8[3] [1041, 1042, 1043]', 'inst_lists': ['<i8[1] [1048]', '<i8[2] [1049, 1050]'],
            'count_mb': '<i8[2, 1] [[1060], [1061]]'}]]],
    'run_cams M=2 rects no boxes':
        [[['lpf_run_cams', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] ff5d7a01baa9', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0,
                       'on_device': 0, 'reserved': 0},
             'corners_velo': 'NULL', 'box_off': 'NULL', 'boxes_on_device': 0, 'oriented': 0},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] 86289c695a6c', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1,
                       'on_device': 0, 'reserved': 0},
             'corners_velo': 'NULL', 'box_off': 'NULL', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'},
            {'uv': 'out[20]', 'label_bits': 'out[10]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]',
             'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'summary': 'out[2] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[20]', 'label_valid': 'out[10]'}]]],
         [[{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
            'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
            'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'valid_idx': '<i8[4] [35, 36, 37, 38]',
            'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]', 'u_valid': '<i4[4] [84, 86, 88, 90]',
            'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'],
            'count_mb': '<i8[2, 0] [[], []]'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
            'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]', 'label_bits': '<u4[4] [13, 14, 15, 16]',
            'depth': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'uf': '<f8[4] [27.0, 28.0, 29.0, 30.0]', 'vf': '<f8[4] [34.0, 35.0, 36.0, 37.0]',
            'valid_idx': '<i8[3] [41, 42, 43]', 'uv_valid': '<i4[3, 2] [[96, 97], [98, 99], [100, 101]]', 'u_valid': '<i4[3] [96, 98, 100]',
            'v_valid': '<i4[3] [97, 99, 101]', 'label_valid': '<u4[3] [97, 98, 99]', 'inst_lists': ['<i8[1] [48]', '<i8[2] [49, 50]'],
            'count_mb': '<i8[2, 0] [[], []]'}],
          [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'label_bits': '<u4[6] [1007, 1008, 1009, 1010, 1011, 1012]', 'depth': '<f8[6] [1014.0, 1015.0, 1016.0, 1017.0, 1018.0, 1019.0]',
            'uf': '<f8[6] [1021.0, 1022.0, 1023.0, 1024.0, 1025.0, 1026.0]', 'vf': '<f8[6] [1028.0, 1029.0, 1030.0, 1031.0, 1032.0, 1033.0]',
            'valid_idx': '<i8[4] [1035, 1036, 1037, 1038]', 'uv_valid': '<i4[4, 2] [[1084, 1085], [1086, 1087], [1088, 1089], [1090, 1091]]',
            'u_valid': '<i4[4] [1084, 1086, 1088, 1090]', 'v_valid': '<i4[4] [1085, 1087, 1089, 1091]',
            'label_valid': '<u4[4] [1091, 1092, 1093, 1094]', 'inst_lists': ['<i8[2] [1042, 1043]', '<i8[1] [1044]'],
            'count_mb': '<i8[2, 0] [[], []]'},
           {'n_valid': 3, 'n_labelled': 1, 'inst_count': '<i8[2] [1, 2]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 7]',
            'u': '<i4[4] [1012, 1014, 1016, 1018]', 'v': '<i4[4] [1013, 1015, 1017, 1019]', 'label_bits': '<u4[4] [1013, 1014, 1015, 1016]',
            'depth': '<f8[4] [1020.0, 1021.0, 1022.0, 1023.0]', 'uf': '<f8[4] [1027.0, 1028.0, 1029.0, 1030.0]',
            'vf': '<f8[4] [1034.0, 1035.0, 1036.0, 1037.0]', 'valid_idx': '<i8[3] [1041, 1042, 1043]',
            'uv_valid': '<i4[3, 2] [[1096, 1097], [1098, 1099], [1100, 1101]]', 'u_valid': '<i4[3] [1096, 1098, 1100]',
            'v_valid': '<i4[3] [1097, 1099, 1101]', 'label_valid': '<u4[3] [1097, 1098, 1099]',
            'inst_lists': ['<i8[1] [1048]', '<i8[2] [1049, 1050]'], 'count_mb': '<i8[2, 0] [[], []]'}]]],
    'run_cams pinned':
        [[['lpf_run_cams', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[6144] c30a70aebf56', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 7b28e5e189bc', 'box_off': 'in[2] 1499246f5a6a', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[6144] c30a70aebf56', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 3daf62e2be56', 'box_off': 'in[2] 1499246f5a6a', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[12]', 'label_bits': 'out[6]', 'depth': 'out[6]', 'u_f': 'out[6]', 'v_f': 'out[6]', 'valid_idx': 'out[6]',
             'inst_idx': 'out[6]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[1] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[12]', 'label_valid': 'out[6]'},
            {'uv': 'out[12]', 'label_bits': 'out[6]', 'depth': 'out[6]', 'u_f': 'out[6]', 'v_f': 'out[6]', 'valid_idx': 'out[6]',
             'inst_idx': 'out[6]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'summary': 'out[1] was all 0', 'on_device': 0, 'reserved': 0,
             'uv_valid': 'out[12]', 'label_valid': 'out[6]'}]]],
         [[{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'label_bits': '<u4[6] [7, 8, 9, 10, 11, 12]',
            'depth': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]', 'uf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]',
            'vf': '<f8[6] [28.0, 29.0, 30.0, 31.0, 32.0, 33.0]', 'valid_idx': '<i8[4] [35, 36, 37, 38]',
            'uv_valid': '<i4[4, 2] [[84, 85], [86, 87], [88, 89], [90, 91]]', 'u_valid': '<i4[4] [84, 86, 88, 90]',
            'v_valid': '<i4[4] [85, 87, 89, 91]', 'label_valid': '<u4[4] [91, 92, 93, 94]', 'inst_lists': ['<i8[2] [42, 43]', '<i8[1] [44]'],
            'count_mb': '<i8[2, 3] [[56, 57, 58], [59, 60, 61]]'}],
          [{'n_valid': 4, 'n_labelled': 2, 'inst_count': '<i8[2] [2, 1]', 'best_box': '<i4[2] [1, -1]', 'best_cnt': '<i8[2] [5, 6]',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'label_bits': '<u4[6] [1007, 1008, 1009, 1010, 1011, 1012]', 'depth': '<f8[6] [1014.0, 1015.0, 1016.0, 1017.0, 1018.0, 1019.0]',
            'uf': '<f8[6] [1021.0, 1022.0, 1023.0, 1024.0, 1025.0, 1026.0]', 'vf': '<f8[6] [1028.0, 1029.0, 1030.0, 1031.0, 1032.0, 1033.0]',
            'valid_idx': '<i8[4] [1035, 1036, 1037, 1038]', 'uv_valid': '<i4[4, 2] [[1084, 1085], [1086, 1087], [1088, 1089], [1090, 1091]]',
            'u_valid': '<i4[4] [1084, 1086, 1088, 1090]', 'v_valid': '<i4[4] [1085, 1087, 1089, 1091]',
            'label_valid': '<u4[4] [1091, 1092, 1093, 1094]', 'inst_lists': ['<i8[2] [1042, 1043]', '<i8[1] [1044]'],
            'count_mb': '<i8[2, 3] [[1056, 1057, 1058], [1059, 1060, 1061]]'}]]],
    'run_cams_wide M=0':
        [[['lpf_run_cams_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0, 'reserved': 0},
             'corners_velo': 'in[72] 6ed0631adb52', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0, 'reserved': 0},
             'corners_velo': 'in[72] d4972ac5f49b', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'NULL',
             'label_valid_words': 'NULL', 'inst_idx': 'NULL', 'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'NULL', 'inst_off': 'out[2] was all 0', 'best_cnt': 'NULL', 'best_box': 'NULL',
             'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0},
            {'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'NULL',
             'label_valid_words': 'NULL', 'inst_idx': 'NULL', 'inst_cap': 6, 'count_mb': 'out[1] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'NULL', 'inst_off': 'out[2] was all 0', 'best_cnt': 'NULL', 'best_box': 'NULL',
             'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'label_words': '<u4[6, 0] [[], [], [], [], [], []]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
            'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': [], 'count_mb': '<i8[0, 2] []'},
           {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'label_words': '<u4[4, 0] [[], [], [], []]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
            'valid_idx': '<i8[3] [34, 35, 36]', 'inst_lists': [], 'count_mb': '<i8[0, 1] []'}],
          [{'n_valid': 4, 'n_labelled': 1084, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'label_words': '<u4[6, 0] [[], [], [], [], [], []]', 'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]',
            'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]', 'valid_idx': '<i8[4] [1028, 1029, 1030, 1031]', 'inst_lists': [],
            'count_mb': '<i8[0, 2] []'},
           {'n_valid': 3, 'n_labelled': 1085, 'inst_count': '<i8[0] []', 'best_box': '<i4[0] []', 'best_cnt': '<i8[0] []',
            'label_words': '<u4[4, 0] [[], [], [], []]', 'u': '<i4[4] [1012, 1014, 1016, 1018]', 'v': '<i4[4] [1013, 1015, 1017, 1019]',
            'valid_idx': '<i8[3] [1034, 1035, 1036]', 'inst_lists': [], 'count_mb': '<i8[0, 1] []'}]]],
    'run_cams_wide M=2':
        [[['lpf_run_cams_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 6ed0631adb52', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] d4972ac5f49b', 'box_off': 'in[3] dbd6951f6833', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0},
            {'uv': 'out[20]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[10]', 'uv_valid': 'NULL', 'label_words': 'out[10]',
             'label_valid_words': 'NULL', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[2] was all 0',
             'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0', 'best_cnt': 'out[4] was all 0',
             'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
            'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
            'valid_idx': '<i8[4] [28, 29, 30, 31]', 'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 2] [[70, 71], [72, 73]]'},
           {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
            'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
            'valid_idx': '<i8[3] [34, 35, 36]', 'inst_lists': ['<i8[1] [62]', '<i8[2] [63, 64]'], 'count_mb': '<i8[2, 1] [[74], [75]]'}],
          [{'n_valid': 4, 'n_labelled': 1084, 'inst_count': '<i8[2] [1091, 1092]', 'best_box': '<i4[2] [1112, 1113]',
            'best_cnt': '<i8[2] [1105, 1106]', 'label_words': '<u4[6, 1] [[1042], [1043], [1044], [1045], [1046], [1047]]',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'valid_idx': '<i8[4] [1028, 1029, 1030, 1031]', 'inst_lists': ['<i8[2] [1056, 1057]', '<i8[1] [1058]'],
            'count_mb': '<i8[2, 2] [[1070, 1071], [1072, 1073]]'},
           {'n_valid': 3, 'n_labelled': 1085, 'inst_count': '<i8[2] [1093, 1094]', 'best_box': '<i4[2] [1114, 1115]',
            'best_cnt': '<i8[2] [1107, 1108]', 'label_words': '<u4[4, 1] [[1048], [1049], [1050], [1051]]', 'u': '<i4[4] [1012, 1014, 1016, 1018]',
            'v': '<i4[4] [1013, 1015, 1017, 1019]', 'valid_idx': '<i8[3] [1034, 1035, 1036]', 'inst_lists': ['<i8[1] [1062]', '<i8[2] [1063, 1064]'],
            'count_mb': '<i8[2, 1] [[1074], [1075]]'}]]],
    'run_cams_wide M=2 rects no boxes':
        [[['lpf_run_cams_wide', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] ff5d7a01baa9', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0,
                       'on_device': 0, 'reserved': 0},
             'corners_velo': 'NULL', 'box_off': 'NULL', 'boxes_on_device': 0, 'oriented': 0},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] 86289c695a6c', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1,
                       'on_device': 0, 'reserved': 0},
             'corners_velo': 'NULL', 'box_off': 'NULL', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[20]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]', 'uv_valid': 'out[20]',
             'label_words': 'out[10]', 'label_valid_words': 'out[10]', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[1] was all 0',
             'n_valid': 'out[2] was all 0', 'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0',
             'best_cnt': 'out[4] was all 0', 'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0},
            {'uv': 'out[20]', 'depth': 'out[10]', 'u_f': 'out[10]', 'v_f': 'out[10]', 'valid_idx': 'out[10]', 'uv_valid': 'out[20]',
             'label_words': 'out[10]', 'label_valid_words': 'out[10]', 'inst_idx': 'out[12]', 'inst_cap': 6, 'count_mb': 'out[1] was all 0',
             'n_valid': 'out[2] was all 0', 'n_labelled': 'out[2] was all 0', 'inst_count': 'out[4] was all 0', 'inst_off': 'out[6] was all 0',
             'best_cnt': 'out[4] was all 0', 'best_box': 'out[4] was all -1', 'inst_overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
            'label_words': '<u4[6, 1] [[42], [43], [44], [45], [46], [47]]', 'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]',
            'depth': '<f8[6] [7.0, 8.0, 9.0, 10.0, 11.0, 12.0]', 'uf': '<f8[6] [14.0, 15.0, 16.0, 17.0, 18.0, 19.0]',
            'vf': '<f8[6] [21.0, 22.0, 23.0, 24.0, 25.0, 26.0]', 'valid_idx': '<i8[4] [28, 29, 30, 31]',
            'uv_valid': '<i4[4, 2] [[35, 36], [37, 38], [39, 40], [41, 42]]', 'u_valid': '<i4[4] [35, 37, 39, 41]',
            'v_valid': '<i4[4] [36, 38, 40, 42]', 'label_valid_words': '<u4[4, 1] [[49], [50], [51], [52]]',
            'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 0] [[], []]'},
           {'n_valid': 3, 'n_labelled': 85, 'inst_count': '<i8[2] [93, 94]', 'best_box': '<i4[2] [114, 115]', 'best_cnt': '<i8[2] [107, 108]',
            'label_words': '<u4[4, 1] [[48], [49], [50], [51]]', 'u': '<i4[4] [12, 14, 16, 18]', 'v': '<i4[4] [13, 15, 17, 19]',
            'depth': '<f8[4] [13.0, 14.0, 15.0, 16.0]', 'uf': '<f8[4] [20.0, 21.0, 22.0, 23.0]', 'vf': '<f8[4] [27.0, 28.0, 29.0, 30.0]',
            'valid_idx': '<i8[3] [34, 35, 36]', 'uv_valid': '<i4[3, 2] [[47, 48], [49, 50], [51, 52]]', 'u_valid': '<i4[3] [47, 49, 51]',
            'v_valid': '<i4[3] [48, 50, 52]', 'label_valid_words': '<u4[3, 1] [[55], [56], [57]]', 'inst_lists': ['<i8[1] [62]', '<i8[2] [63, 64]'],
            'count_mb': '<i8[2, 0] [[], []]'}],
          [{'n_valid': 4, 'n_labelled': 1084, 'inst_count': '<i8[2] [1091, 1092]', 'best_box': '<i4[2] [1112, 1113]',
            'best_cnt': '<i8[2] [1105, 1106]', 'label_words': '<u4[6, 1] [[1042], [1043], [1044], [1045], [1046], [1047]]',
            'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'depth': '<f8[6] [1007.0, 1008.0, 1009.0, 1010.0, 1011.0, 1012.0]', 'uf': '<f8[6] [1014.0, 1015.0, 1016.0, 1017.0, 1018.0, 1019.0]',
            'vf': '<f8[6] [1021.0, 1022.0, 1023.0, 1024.0, 1025.0, 1026.0]', 'valid_idx': '<i8[4] [1028, 1029, 1030, 1031]',
            'uv_valid': '<i4[4, 2] [[1035, 1036], [1037, 1038], [1039, 1040], [1041, 1042]]', 'u_valid': '<i4[4] [1035, 1037, 1039, 1041]',
            'v_valid': '<i4[4] [1036, 1038, 1040, 1042]', 'label_valid_words': '<u4[4, 1] [[1049], [1050], [1051], [1052]]',
            'inst_lists': ['<i8[2] [1056, 1057]', '<i8[1] [1058]'], 'count_mb': '<i8[2, 0] [[], []]'},
           {'n_valid': 3, 'n_labelled': 1085, 'inst_count': '<i8[2] [1093, 1094]', 'best_box': '<i4[2] [1114, 1115]',
            'best_cnt': '<i8[2] [1107, 1108]', 'label_words': '<u4[4, 1] [[1048], [1049], [1050], [1051]]', 'u': '<i4[4] [1012, 1014, 1016, 1018]',
            'v': '<i4[4] [1013, 1015, 1017, 1019]', 'depth': '<f8[4] [1013.0, 1014.0, 1015.0, 1016.0]',
            'uf': '<f8[4] [1020.0, 1021.0, 1022.0, 1023.0]', 'vf': '<f8[4] [1027.0, 1028.0, 1029.0, 1030.0]',
            'valid_idx': '<i8[3] [1034, 1035, 1036]', 'uv_valid': '<i4[3, 2] [[1047, 1048], [1049, 1050], [1051, 1052]]',
            'u_valid': '<i4[3] [1047, 1049, 1051]', 'v_valid': '<i4[3] [1048, 1050, 1052]', 'label_valid_words': '<u4[3, 1] [[1055], [1056], [1057]]',
            'inst_lists': ['<i8[1] [1062]', '<i8[2] [1063, 1064]'], 'count_mb': '<i8[2, 0] [[], []]'}]]],
    'run_cams_wide pinned no label':
        [[['lpf_run_cams_wide', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'T_velo_to_rect': [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0],
             'K': [2.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 2.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 40.0,
             'masks': {'masks': 'in[6144] c30a70aebf56', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 0, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 7b28e5e189bc', 'box_off': 'in[2] 1499246f5a6a', 'boxes_on_device': 0, 'oriented': 1},
            {'T_velo_to_rect': [2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0, 1.0, 2.0],
             'K': [3.0, 0.0, 0.0, 0.0, 3.0, 0.0, 0.0, 0.0, 3.0], 'W': 64, 'H': 48, 'depth_min_excl': 0.0, 'depth_max_excl': 41.0,
             'masks': {'masks': 'in[6144] c30a70aebf56', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 0, 'erode_iters': 1, 'on_device': 0,
                       'reserved': 0},
             'corners_velo': 'in[72] 3daf62e2be56', 'box_off': 'in[2] 1499246f5a6a', 'boxes_on_device': 0, 'oriented': 0}],
           2,
           [{'uv': 'out[12]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[6]', 'uv_valid': 'out[12]', 'label_words': 'NULL',
             'label_valid_words': 'out[6]', 'inst_idx': 'out[6]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[1] was all 0',
             'n_labelled': 'out[1] was all 0', 'inst_count': 'out[2] was all 0', 'inst_off': 'out[3] was all 0', 'best_cnt': 'out[2] was all 0',
             'best_box': 'out[2] was all -1', 'inst_overflow': 'out[1] was all 0', 'on_device': 0, 'reserved': 0},
            {'uv': 'out[12]', 'depth': 'NULL', 'u_f': 'NULL', 'v_f': 'NULL', 'valid_idx': 'out[6]', 'uv_valid': 'out[12]', 'label_words': 'NULL',
             'label_valid_words': 'out[6]', 'inst_idx': 'out[6]', 'inst_cap': 6, 'count_mb': 'out[6] was all 0', 'n_valid': 'out[1] was all 0',
             'n_labelled': 'out[1] was all 0', 'inst_count': 'out[2] was all 0', 'inst_off': 'out[3] was all 0', 'best_cnt': 'out[2] was all 0',
             'best_box': 'out[2] was all -1', 'inst_overflow': 'out[1] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[{'n_valid': 4, 'n_labelled': 84, 'inst_count': '<i8[2] [91, 92]', 'best_box': '<i4[2] [112, 113]', 'best_cnt': '<i8[2] [105, 106]',
            'u': '<i4[6] [0, 2, 4, 6, 8, 10]', 'v': '<i4[6] [1, 3, 5, 7, 9, 11]', 'valid_idx': '<i8[4] [28, 29, 30, 31]',
            'uv_valid': '<i4[4, 2] [[35, 36], [37, 38], [39, 40], [41, 42]]', 'u_valid': '<i4[4] [35, 37, 39, 41]',
            'v_valid': '<i4[4] [36, 38, 40, 42]', 'label_valid_words': '<u4[4, 1] [[49], [50], [51], [52]]',
            'inst_lists': ['<i8[2] [56, 57]', '<i8[1] [58]'], 'count_mb': '<i8[2, 3] [[70, 71, 72], [73, 74, 75]]'}],
          [{'n_valid': 4, 'n_labelled': 1084, 'inst_count': '<i8[2] [1091, 1092]', 'best_box': '<i4[2] [1112, 1113]',
            'best_cnt': '<i8[2] [1105, 1106]', 'u': '<i4[6] [1000, 1002, 1004, 1006, 1008, 1010]', 'v': '<i4[6] [1001, 1003, 1005, 1007, 1009, 1011]',
            'valid_idx': '<i8[4] [1028, 1029, 1030, 1031]', 'uv_valid': '<i4[4, 2] [[1035, 1036], [1037, 1038], [1039, 1040], [1041, 1042]]',
            'u_valid': '<i4[4] [1035, 1037, 1039, 1041]', 'v_valid': '<i4[4] [1036, 1038, 1040, 1042]',
            'label_valid_words': '<u4[4, 1] [[1049], [1050], [1051], [1052]]', 'inst_lists': ['<i8[2] [1056, 1057]', '<i8[1] [1058]'],
            'count_mb': '<i8[2, 3] [[1070, 1071, 1072], [1073, 1074, 1075]]'}]]],
    'depth_maps':
        [[['lpf_depth_maps', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 2, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'pix': 'out[8]', 'depth': 'out[8]', 'point_idx': 'out[8]', 'cap': 4, 'car_off': 'out[6] was all 0', 'need': 'out[2] was all 0',
             'overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[['<i8[1] [0]', '<f8[1] [7.0]', '<i8[1] [14]'], ['<i8[2] [1, 2]', '<f8[2] [8.0, 9.0]', '<i8[2] [15, 16]']],
          [['<i8[2] [4, 5]', '<f8[2] [11.0, 12.0]', '<i8[2] [18, 19]'], ['<i8[0] []', '<f8[0] []', '<i8[0] []']]]],
    'depth_maps default cap F=1':
        [[['lpf_depth_maps', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'masks': 'in[6144] c30a70aebf56', 'rects': 'NULL', 'M': 2, 'f32': 0, 'binarize': 2, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'pix': 'out[1024]', 'depth': 'out[1024]', 'point_idx': 'out[1024]', 'cap': 1024, 'car_off': 'out[3] was all 0',
             'need': 'out[1] was all 0', 'overflow': 'out[1] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[['<i8[1] [0]', '<f8[1] [7.0]', '<i8[1] [14]'], ['<i8[2] [1, 2]', '<f8[2] [8.0, 9.0]', '<i8[2] [15, 16]']]]],
    'depth_maps M=0':
        [[['lpf_depth_maps', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'NULL', 'rects': 'NULL', 'M': 0, 'f32': 0, 'binarize': 2, 'erode_iters': 0, 'on_device': 0, 'reserved': 0}],
           [{'pix': 'NULL', 'depth': 'NULL', 'point_idx': 'NULL', 'cap': 0, 'car_off': 'out[2] was all 0', 'need': 'out[2] was all 0',
             'overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[], []]],
    'depth_maps overflow':
        [[['lpf_depth_maps', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] ff5d7a01baa9', 'M': 2, 'f32': 0, 'binarize': 2, 'erode_iters': 1, 'on_device': 0,
             'reserved': 0}],
           [{'pix': 'out[8]', 'depth': 'out[8]', 'point_idx': 'NULL', 'cap': 4, 'car_off': 'out[6] was all 0', 'need': 'out[2] was all 0',
             'overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]],
          ['lpf_depth_maps', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'masks': 'in[12288] 647fe3966066', 'rects': 'in[16] ff5d7a01baa9', 'M': 2, 'f32': 0, 'binarize': 2, 'erode_iters': 1, 'on_device': 0,
             'reserved': 0}],
           [{'pix': 'out[14]', 'depth': 'out[14]', 'point_idx': 'NULL', 'cap': 7, 'car_off': 'out[6] was all 0', 'need': 'out[2] was all 0',
             'overflow': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [[['<i8[1] [0]', '<f8[1] [7.0]', None], ['<i8[2] [1, 2]', '<f8[2] [8.0, 9.0]', None]],
          [['<i8[2] [7, 8]', '<f8[2] [14.0, 15.0]', None], ['<i8[0] []', '<f8[0] []', None]]]],
    'depth_overlays':
        [[['lpf_depth_overlays', 2,
           [{'pix': 'in[12] 99b1a4c6d69b', 'depth': 'in[12] fca60e5fb70d', 'cap': 6, 'car_off': 'in[6] 1929a12aa8ae', 'M': 2, 'lists_on_device': 0,
             'seg': 'in[18432] a15ed5a8e541', 'seg_on_device': 0, 'reserved': 0}],
           [{'images': 'out[36864]', 'max_depth': 'out[4] was all 0.0', 'on_device': 0, 'reserved': 0}]]],
         ['|u1[2, 2, 48, 64, 3] 3b55c51c8819', '<f8[2, 2] [[7.0, 8.0], [9.0, 10.0]]']],
    'depth_overlays F=1':
        [[['lpf_depth_overlays', 1,
           [{'pix': 'in[3] e422a5107c33', 'depth': 'in[3] 443472c743bd', 'cap': 3, 'car_off': 'in[3] ba09b3dfd9c4', 'M': 2, 'lists_on_device': 0,
             'seg': 'in[9216] 3a111374cc75', 'seg_on_device': 0, 'reserved': 0}],
           [{'images': 'out[18432]', 'max_depth': 'out[2] was all 0.0', 'on_device': 0, 'reserved': 0}]]],
         ['|u1[1, 2, 48, 64, 3] 9133f2aad841', '<f8[1, 2] [[7.0, 8.0]]']],
    'depth_overlays M=0':
        [[], ['|u1[2, 0, 48, 64, 3] [[], []]', '<f8[2, 0] [[], []]']],
    'match_2d best':
        [[['lpf_match_2d', 2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.25, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'best_box': 'out[3] was all -1', 'best_iou': 'out[3] was all 0.0', 'iou': 'NULL', 'center_score': 'NULL', 'size_score': 'NULL',
             'total_score': 'NULL', 'cost': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'best_box': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'best_iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]']}],
    'match_2d one matrix':
        [[['lpf_match_2d', 2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.25, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'best_box': 'NULL', 'best_iou': 'NULL', 'iou': 'NULL', 'center_score': 'out[5]', 'size_score': 'NULL', 'total_score': 'NULL',
             'cost': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'center': ['<f8[2, 2] [[21.0, 22.0], [23.0, 24.0]]', '<f8[1, 1] [[25.0]]']}],
    'match_2d everything':
        [[['lpf_match_2d', 2,
           [{'dets': 'in[24] 39ea56ef0b82', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 1, 'on_device': 0, 'min_iou': 0.5, 'w_iou': 0.25, 'w_center': 0.5, 'w_size': 0.125}],
           [{'best_box': 'out[3] was all -1', 'best_iou': 'out[3] was all 0.0', 'iou': 'out[5]', 'center_score': 'out[5]', 'size_score': 'out[5]',
             'total_score': 'out[5]', 'cost': 'out[5]', 'on_device': 0, 'reserved': 0}]]],
         {'best_box': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'best_iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]'],
          'iou': ['<f8[2, 2] [[14.0, 15.0], [16.0, 17.0]]', '<f8[1, 1] [[18.0]]'],
          'center': ['<f8[2, 2] [[21.0, 22.0], [23.0, 24.0]]', '<f8[1, 1] [[25.0]]'],
          'size': ['<f8[2, 2] [[28.0, 29.0], [30.0, 31.0]]', '<f8[1, 1] [[32.0]]'],
          'total': ['<f8[2, 2] [[35.0, 36.0], [37.0, 38.0]]', '<f8[1, 1] [[39.0]]'],
          'cost': ['<f8[2, 2] [[42.0, 43.0], [44.0, 45.0]]', '<f8[1, 1] [[46.0]]']}],
    'match_2d F=1':
        [[['lpf_match_2d', 1,
           [{'dets': 'in[8] a00dc06e2530', 'det_off': 'in[2] 391dabcb730f', 'bbox2d': 'in[12] dd81ba74486e', 'front': 'in[3] 727432515ae3',
             'box_off': 'in[2] 1499246f5a6a', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.25, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'best_box': 'out[2] was all -1', 'best_iou': 'out[2] was all 0.0', 'iou': 'NULL', 'center_score': 'NULL', 'size_score': 'NULL',
             'total_score': 'NULL', 'cost': 'out[6]', 'on_device': 0, 'reserved': 0}]]],
         {'best_box': ['<i4[2] [0, 1]'], 'best_iou': ['<f8[2] [7.0, 8.0]'], 'cost': ['<f8[2, 3] [[42.0, 43.0, 44.0], [45.0, 46.0, 47.0]]']}],
    'match_2d no detections':
        [[], {'best_box': ['<i4[0] []', '<i4[0] []'], 'best_iou': ['<f8[0] []', '<f8[0] []'], 'iou': ['<f8[0, 2] []', '<f8[0, 1] []']}],
    'match_2d no boxes':
        [[['lpf_match_2d', 2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'NULL', 'front': 'NULL', 'box_off': 'in[3] 2c513f149e73',
             'dets_f64': 0, 'on_device': 0, 'min_iou': 0.25, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'best_box': 'out[3] was all -1', 'best_iou': 'out[3] was all 0.0', 'iou': 'NULL', 'center_score': 'NULL', 'size_score': 'NULL',
             'total_score': 'NULL', 'cost': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'best_box': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'best_iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]'],
          'iou': ['<f8[2, 0] [[], []]', '<f8[1, 0] [[]]']}],
    'assign_costs':
        [[['lpf_assign_costs',
           2,
           [{'cost': 'in[9] 8a90cc92f878', 'det_off': 'in[3] be73167ff39f', 'box_off': 'in[3] 4b9e096d5cbe', 'front': 'NULL', 'on_device': 0,
             'reserved': 0}],
           [{'col_of_row': 'out[5] was all -1', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [['<i8[1] [1]', '<i8[1] [0]'], ['<i8[2] [0, 2]', '<i8[2] [1, 0]']]],
    'assign_costs front':
        [[['lpf_assign_costs',
           2,
           [{'cost': 'in[9] 8a90cc92f878', 'det_off': 'in[3] be73167ff39f', 'box_off': 'in[3] 4b9e096d5cbe', 'front': 'in[4] d862455f3f46',
             'on_device': 0, 'reserved': 0}],
           [{'col_of_row': 'out[5] was all -1', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [['<i8[1] [1]', '<i8[1] [0]'], ['<i8[2] [0, 2]', '<i8[2] [1, 0]']]],
    'assign_costs raw':
        [[['lpf_assign_costs',
           2,
           [{'cost': 'in[9] 8a90cc92f878', 'det_off': 'in[3] be73167ff39f', 'box_off': 'in[3] 4b9e096d5cbe', 'front': 'NULL', 'on_device': 0,
             'reserved': 0}],
           [{'col_of_row': 'out[5] was all -1', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'col_of_row': '<i4[5] [-1, 0, 1, -1, 0]', 'status': '<i4[2] [0, 0]'}],
    'assign_costs F=1':
        [[['lpf_assign_costs',
           1,
           [{'cost': 'in[6] de6a6a2af671', 'det_off': 'in[2] 391dabcb730f', 'box_off': 'in[2] 1499246f5a6a', 'front': 'NULL', 'on_device': 0,
             'reserved': 0}],
           [{'col_of_row': 'out[2] was all -1', 'status': 'out[1] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [['<i8[1] [1]', '<i8[1] [0]']]],
    'assign_costs no rows, no columns':
        [[['lpf_assign_costs',
           2,
           [{'cost': 'NULL', 'det_off': 'in[3] 0c38220b7676', 'box_off': 'in[3] 3f5d427fff4f', 'front': 'in[3] 727432515ae3', 'on_device': 0,
             'reserved': 0}],
           [{'col_of_row': 'out[2] was all -1', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         [['<i8[0] []', '<i8[0] []'], ['<i8[1] [1]', '<i8[1] [0]']]],
    'assign_costs a frame without an assignment':
        [[['lpf_assign_costs',
           2,
           [{'cost': 'in[9] 8a90cc92f878', 'det_off': 'in[3] be73167ff39f', 'box_off': 'in[3] 4b9e096d5cbe', 'front': 'NULL', 'on_device': 0,
             'reserved': 0}],
           [{'col_of_row': 'out[5] was all -1', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         'ValueError: assign_costs: frame 1: cost matrix is infeasible'],
    'assign_2d':
        [[['lpf_assign_2d',
           2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'min_score_threshold': 0.3, 'min_iou_threshold': 0.15}],
           [{'box_of_det': 'out[3] was all -1', 'iou': 'out[3] was all 0.0', 'center_score': 'out[3] was all 0.0', 'size_score': 'out[3] was all 0.0',
             'total_score': 'out[3] was all 0.0', 'accepted': 'out[3] was all 0', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]'],
          'center': ['<f8[2] [14.0, 15.0]', '<f8[1] [16.0]'], 'size': ['<f8[2] [21.0, 22.0]', '<f8[1] [23.0]'],
          'total': ['<f8[2] [28.0, 29.0]', '<f8[1] [30.0]'], 'accepted': ['<i4[2] [35, 36]', '<i4[1] [37]'], 'status': '<i4[2] [42, 43]'}],
    'assign_2d float64':
        [[['lpf_assign_2d',
           2,
           [{'dets': 'in[24] 39ea56ef0b82', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 1, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.25, 'w_center': 0.5, 'w_size': 0.125}],
           [{'min_score_threshold': 0.5, 'min_iou_threshold': 0.125}],
           [{'box_of_det': 'out[3] was all -1', 'iou': 'out[3] was all 0.0', 'center_score': 'out[3] was all 0.0', 'size_score': 'out[3] was all 0.0',
             'total_score': 'out[3] was all 0.0', 'accepted': 'out[3] was all 0', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]'],
          'center': ['<f8[2] [14.0, 15.0]', '<f8[1] [16.0]'], 'size': ['<f8[2] [21.0, 22.0]', '<f8[1] [23.0]'],
          'total': ['<f8[2] [28.0, 29.0]', '<f8[1] [30.0]'], 'accepted': ['<i4[2] [35, 36]', '<i4[1] [37]'], 'status': '<i4[2] [42, 43]'}],
    'assign_2d two outputs':
        [[['lpf_assign_2d',
           2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'min_score_threshold': 0.3, 'min_iou_threshold': 0.15}],
           [{'box_of_det': 'out[3] was all -1', 'iou': 'NULL', 'center_score': 'NULL', 'size_score': 'NULL', 'total_score': 'NULL', 'accepted': 'NULL',
             'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'status': '<i4[2] [42, 43]'}],
    'assign_2d F=1':
        [[['lpf_assign_2d',
           1,
           [{'dets': 'in[8] a00dc06e2530', 'det_off': 'in[2] 391dabcb730f', 'bbox2d': 'in[12] dd81ba74486e', 'front': 'in[3] 727432515ae3',
             'box_off': 'in[2] 1499246f5a6a', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'min_score_threshold': 0.3, 'min_iou_threshold': 0.15}],
           [{'box_of_det': 'out[2] was all -1', 'iou': 'out[2] was all 0.0', 'center_score': 'out[2] was all 0.0', 'size_score': 'out[2] was all 0.0',
             'total_score': 'out[2] was all 0.0', 'accepted': 'out[2] was all 0', 'status': 'out[1] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[2] [0, 1]'], 'iou': ['<f8[2] [7.0, 8.0]'], 'center': ['<f8[2] [14.0, 15.0]'], 'size': ['<f8[2] [21.0, 22.0]'],
          'total': ['<f8[2] [28.0, 29.0]'], 'accepted': ['<i4[2] [35, 36]'], 'status': '<i4[1] [42]'}],
    'assign_2d no detections':
        [[['lpf_assign_2d',
           2,
           [{'dets': 'NULL', 'det_off': 'in[3] 2c513f149e73', 'bbox2d': 'in[12] a6a44d538b13', 'front': 'in[3] 43f1e6e3bac3',
             'box_off': 'in[3] dbd6951f6833', 'dets_f64': 0, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'min_score_threshold': 0.3, 'min_iou_threshold': 0.15}],
           [{'box_of_det': 'NULL', 'iou': 'NULL', 'center_score': 'NULL', 'size_score': 'NULL', 'total_score': 'NULL', 'accepted': 'NULL',
             'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[0] []', '<i4[0] []'], 'iou': ['<f8[0] []', '<f8[0] []'], 'center': ['<f8[0] []', '<f8[0] []'],
          'size': ['<f8[0] []', '<f8[0] []'], 'total': ['<f8[0] []', '<f8[0] []'], 'accepted': ['<i4[0] []', '<i4[0] []'], 'status': '<i4[2] [42, 43]'}],
    'assign_2d no boxes':
        [[['lpf_assign_2d',
           2,
           [{'dets': 'in[12] cb3910689d7e', 'det_off': 'in[3] dbd6951f6833', 'bbox2d': 'NULL', 'front': 'NULL', 'box_off': 'in[3] 2c513f149e73',
             'dets_f64': 0, 'on_device': 0, 'min_iou': 0.0, 'w_iou': 0.5, 'w_center': 0.3, 'w_size': 0.2}],
           [{'min_score_threshold': 0.3, 'min_iou_threshold': 0.15}],
           [{'box_of_det': 'out[3] was all -1', 'iou': 'out[3] was all 0.0', 'center_score': 'out[3] was all 0.0', 'size_score': 'out[3] was all 0.0',
             'total_score': 'out[3] was all 0.0', 'accepted': 'out[3] was all 0', 'status': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_of_det': ['<i4[2] [0, 1]', '<i4[1] [2]'], 'iou': ['<f8[2] [7.0, 8.0]', '<f8[1] [9.0]'],
          'center': ['<f8[2] [14.0, 15.0]', '<f8[1] [16.0]'], 'size': ['<f8[2] [21.0, 22.0]', '<f8[1] [23.0]'],
          'total': ['<f8[2] [28.0, 29.0]', '<f8[1] [30.0]'], 'accepted': ['<i4[2] [35, 36]', '<i4[1] [37]'], 'status': '<i4[2] [42, 43]'}],
    'inside_masks inside':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'out[10] was all 0', 'part_idx': 'NULL', 'part_xyz': 'NULL', 'n_inside': 'NULL', 'matched': 'NULL', 'on_device': 0,
             'reserved': 0}]]],
         {'inside': '|u1[2, 5] [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]'}],
    'inside_masks part_idx':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'NULL', 'part_idx': 'out[10] was all 0', 'part_xyz': 'NULL', 'n_inside': 'NULL', 'matched': 'NULL', 'on_device': 0,
             'reserved': 0}]]],
         {'part_idx': '<i8[2, 5] [[7, 8, 9, 10, 11], [12, 13, 14, 15, 16]]'}],
    'inside_masks part_xyz':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'NULL', 'part_idx': 'NULL', 'part_xyz': 'out[30] was all 0.0', 'n_inside': 'NULL', 'matched': 'NULL', 'on_device': 0,
             'reserved': 0}]]],
         {'part_xyz': '<f4[2, 5, 3] 68a3d6310773'}],
    'inside_masks n_inside':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'NULL', 'part_idx': 'NULL', 'part_xyz': 'NULL', 'n_inside': 'out[4] was all 0', 'matched': 'NULL', 'on_device': 0,
             'reserved': 0}]]],
         {'n_inside': '<i8[2, 2] [[21, 22], [23, 24]]'}],
    'inside_masks matched':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'NULL', 'part_idx': 'NULL', 'part_xyz': 'NULL', 'n_inside': 'NULL', 'matched': 'out[4] was all 0', 'on_device': 0,
             'reserved': 0}]]],
         {'matched': '<i4[2, 2] [[28, 29], [30, 31]]'}],
    'inside_masks all':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 3, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'out[10] was all 0', 'part_idx': 'out[10] was all 0', 'part_xyz': 'out[30] was all 0.0', 'n_inside': 'out[4] was all 0',
             'matched': 'out[4] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'inside': '|u1[2, 5] [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]', 'part_idx': '<i8[2, 5] [[7, 8, 9, 10, 11], [12, 13, 14, 15, 16]]',
          'part_xyz': '<f4[2, 5, 3] 68a3d6310773', 'n_inside': '<i8[2, 2] [[21, 22], [23, 24]]', 'matched': '<i4[2, 2] [[28, 29], [30, 31]]'}],
    'inside_masks F=1':
        [[['lpf_inside_masks', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'inst_idx': 'in[5] bb0517fc301c', 'inst_cap': 5, 'inst_off': 'in[3] f0a0f8394375', 'best_box': 'in[2] cee0539bc356',
             'best_cnt': 'in[2] 12abe15f3d82', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'out[5] was all 0', 'part_idx': 'out[5] was all 0', 'part_xyz': 'out[15] was all 0.0', 'n_inside': 'out[2] was all 0',
             'matched': 'out[2] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'inside': '|u1[1, 5] [[0, 1, 2, 3, 4]]', 'part_idx': '<i8[1, 5] [[7, 8, 9, 10, 11]]', 'part_xyz': '<f4[1, 5, 3] 1f2cae99987d',
          'n_inside': '<i8[1, 2] [[21, 22]]', 'matched': '<i4[1, 2] [[28, 29]]'}],
    'inside_masks out':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'out[10] was all 5', 'part_idx': 'out[10] was all 5', 'part_xyz': 'out[30] was all 0.0', 'n_inside': 'out[4] was all 0',
             'matched': 'out[4] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'inside': '|u1[2, 5] [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]', 'part_idx': '<i8[2, 5] [[7, 8, 9, 10, 11], [12, 13, 14, 15, 16]]',
          'part_xyz': '<f4[2, 5, 3] 68a3d6310773', 'n_inside': '<i8[2, 2] [[21, 22], [23, 24]]', 'matched': '<i4[2, 2] [[28, 29], [30, 31]]'}],
    'inside_masks staged':
        [[['lpf_inside_masks', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'inst_idx': 'in[10] 7edd5894cbbf', 'inst_cap': 5, 'inst_off': 'in[6] 4d626ca2d8bf', 'best_box': 'in[4] 8b58583b8ad1',
             'best_cnt': 'in[4] ca036923ed4f', 'M': 2, 'min_points': 10, 'on_device': 0, 'reserved': 0}],
           [{'inside': 'out[10] was all 0', 'part_idx': 'out[10] was all 0', 'part_xyz': 'out[30] was all 0.0', 'n_inside': 'out[4] was all 0',
             'matched': 'out[4] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'inside': '|u1[2, 5] [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]', 'part_idx': '<i8[2, 5] [[7, 8, 9, 10, 11], [12, 13, 14, 15, 16]]',
          'part_xyz': '<f4[2, 5, 3] 68a3d6310773', 'n_inside': '<i8[2, 2] [[21, 22], [23, 24]]', 'matched': '<i4[2, 2] [[28, 29], [30, 31]]'}],
    'box_points box_points':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'NULL', 'first_box': 'NULL', 'frame_counts': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]'}],
    'box_points box_labelled':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'NULL', 'box_labelled': 'out[3] was all 0', 'first_box': 'NULL', 'frame_counts': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'box_labelled': '<i4[3] [7, 8, 9]'}],
    'box_points first_box':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'NULL', 'box_labelled': 'NULL', 'first_box': 'out[10] was all -1', 'frame_counts': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]'}],
    'box_points frame_counts':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'NULL', 'box_labelled': 'NULL', 'first_box': 'NULL', 'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points all':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'out[10] was all -1',
             'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]',
          'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points out':
        [[['lpf_box_points', 1, 0, [0, 6], '92a5f0f75a8c',
           [{'valid_idx': 'in[6] e0bfa7c7d96f', 'n_valid': 'in[1] f4533a73e647', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'out[3] was all 5', 'box_labelled': 'out[3] was all 5', 'first_box': 'out[6] was all -1',
             'frame_counts': 'out[4] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[6] [14, 15, 16, 17, 18, 19]',
          'frame_counts': '<i8[1, 4] [[21, 22, 23, 24]]'}],
    'box_points staged':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'NULL', 'LW': 0, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'out[10] was all -1',
             'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]',
          'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points label [N]':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'in[10] 14e5d7998793', 'LW': 1, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'out[10] was all -1',
             'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]',
          'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points label [N,1]':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'in[10] 14e5d7998793', 'LW': 1, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'out[10] was all -1',
             'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]',
          'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points label [N,2]':
        [[['lpf_box_points', 2, 0, [0, 6, 10], 'efcda280bd2d',
           [{'valid_idx': 'in[10] d5835647f378', 'n_valid': 'in[2] 812f69557ed3', 'label_valid_words': 'in[20] f4be649721f8', 'LW': 2, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'out[10] was all -1',
             'frame_counts': 'out[8] was all 0', 'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[10] [14, 15, 16, 17, 18, 19, 20, 21, 22, 23]',
          'frame_counts': '<i8[2, 4] [[21, 22, 23, 24], [25, 26, 27, 28]]'}],
    'box_points Ntot=0':
        [[['lpf_box_points', 1, 0, [0, 0], 'NULL',
           [{'valid_idx': 'in[1] 05fe40575316', 'n_valid': 'in[1] f4533a73e647', 'label_valid_words': 'NULL', 'LW': 1, 'on_device': 0}],
           [{'box_points': 'out[3] was all 0', 'box_labelled': 'out[3] was all 0', 'first_box': 'NULL', 'frame_counts': 'out[4] was all 0',
             'on_device': 0, 'reserved': 0}]]],
         {'box_points': '<i4[3] [0, 1, 2]', 'box_labelled': '<i4[3] [7, 8, 9]', 'first_box': '<i4[0] []',
          'frame_counts': '<i8[1, 4] [[21, 22, 23, 24]]'}],
    'box_views':
        [[['lpf_box_views', 2,
           [{'corners_cam0': 'in[72] eeda4dc1cf92', 'box_off': 'in[3] dbd6951f6833', 'T_cam_to_velo': 'NULL', 'on_device': 0, 'min_points_in_view': 4,
             'depth_lo': 0.1, 'depth_hi': 100.0, 'min_area': 100.0}],
           [{'keep': 'out[3] was all 0', 'reason': 'out[3] was all 0', 'corners_in_view': 'NULL', 'corners_near': 'NULL', 'avg_depth': 'NULL',
             'near_bbox2d': 'NULL', 'front': 'NULL', 'bbox2d': 'NULL', 'front_avg_depth': 'NULL', 'kept_pos': 'NULL', 'frame_counts': 'NULL',
             'corners_velo': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'keep': '|u1[3] [0, 1, 2]', 'reason': '<i4[3] [7, 8, 9]'}],
    'box_views T':
        [[['lpf_box_views', 2,
           [{'corners_cam0': 'in[72] eeda4dc1cf92', 'box_off': 'in[3] dbd6951f6833', 'T_cam_to_velo': 'in[16] 5b9d2cde5f7c', 'on_device': 0,
             'min_points_in_view': 2, 'depth_lo': 0.5, 'depth_hi': 80.0, 'min_area': 50.0}],
           [{'keep': 'out[3] was all 0', 'reason': 'out[3] was all 0', 'corners_in_view': 'out[3] was all 0', 'corners_near': 'out[3] was all 0',
             'avg_depth': 'out[3] was all 0.0', 'near_bbox2d': 'out[12] was all 0.0', 'front': 'out[3] was all 0', 'bbox2d': 'out[12] was all 0.0',
             'front_avg_depth': 'out[3] was all 0.0', 'kept_pos': 'out[3] was all 0', 'frame_counts': 'out[12] was all 0',
             'corners_velo': 'out[72] was all 0.0', 'on_device': 0, 'reserved': 0}]]],
         {'keep': '|u1[3] [0, 1, 2]', 'reason': '<i4[3] [7, 8, 9]', 'corners_in_view': '<i4[3] [14, 15, 16]', 'corners_near': '<i4[3] [21, 22, 23]',
          'avg_depth': '<f8[3] [28.0, 29.0, 30.0]',
          'near_bbox2d': '<f8[3, 4] [[35.0, 36.0, 37.0, 38.0], [39.0, 40.0, 41.0, 42.0], [43.0, 44.0, 45.0, 46.0]]', 'front': '<i4[3] [42, 43, 44]',
          'bbox2d': '<f8[3, 4] [[49.0, 50.0, 51.0, 52.0], [53.0, 54.0, 55.0, 56.0], [57.0, 58.0, 59.0, 60.0]]',
          'front_avg_depth': '<f8[3] [56.0, 57.0, 58.0]', 'kept_pos': '<i4[3] [63, 64, 65]',
          'frame_counts': '<i4[2, 6] [[70, 71, 72, 73, 74, 75], [76, 77, 78, 79, 80, 81]]', 'corners_velo': '<f8[3, 8, 3] ad34accdb957'}],
    'box_views frame_counts':
        [[['lpf_box_views', 2,
           [{'corners_cam0': 'in[72] eeda4dc1cf92', 'box_off': 'in[3] dbd6951f6833', 'T_cam_to_velo': 'NULL', 'on_device': 0, 'min_points_in_view': 4,
             'depth_lo': 0.1, 'depth_hi': 100.0, 'min_area': 100.0}],
           [{'keep': 'NULL', 'reason': 'NULL', 'corners_in_view': 'NULL', 'corners_near': 'NULL', 'avg_depth': 'NULL', 'near_bbox2d': 'NULL',
             'front': 'NULL', 'bbox2d': 'NULL', 'front_avg_depth': 'NULL', 'kept_pos': 'NULL', 'frame_counts': 'out[12] was all 0',
             'corners_velo': 'NULL', 'on_device': 0, 'reserved': 0}]]],
         {'frame_counts': '<i4[2, 6] [[70, 71, 72, 73, 74, 75], [76, 77, 78, 79, 80, 81]]'}],
}
