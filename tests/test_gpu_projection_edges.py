"""The edge-value projection cases of tests/projection_cases.py through every route of the library that projects: the project+label
tiles in each label source (packed host masks, lent masks gathered directly, lent masks gated by their rectangles, the candidate grid
of the large launches, which projects a second time), in the serial and the software-pipelined launches and under every forced launch
geometry; lpf_run_frame; the wide and multi-camera passes; the depth image and the depth maps; and the three box routes plus
lpf_box_views on the cam-0 corner sets.  The reference is the C oracle (orc.run, orc.depth_image) and tests/box_views_ref.py, which
tests/test_projection_cases.py holds against the exact restatement on the same cases.  Integer outputs are compared bit for bit, float
outputs as bit patterns -- the sign of a zero included -- with NaN by position."""
import numpy as np
import pytest

import box_views_ref as bv
import projection_cases as P
import wide_fuzz_cases as G
from conftest import context_for_form, load_calib
from lidar_object_detection_amd._native import LpfContext, SUMMARY_DTYPE
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp
from test_gpu_depth_maps import _expect, _same as _same_maps
from test_gpu_frame_wide import _host, _outs
from test_gpu_fuzz_wide import _frame_wide_result

pytestmark = pytest.mark.gpu

CALIB = load_calib()
CAMS = P.cameras(CALIB)
NAMES = [c["name"] for c in CAMS]
INDEX = pytest.mark.parametrize("index", range(len(CAMS)), ids=NAMES)
FLOATS = ("depth", "uf", "vf")
EXACT = ("u", "v", "label_bits", "valid_idx", "inst_count", "count_mb", "best_box", "best_cnt", "u_valid", "v_valid", "label_valid")
M_WIDE = 33
_cases = {}


class _Case:
    """one camera's batch -- an empty frame, E alone, the full cloud -- its three masks with their tight rectangles, its boxes, and the
    oracle's results, computed once and shared by the tests (nothing writes to them)"""

    def __init__(self, index):
        self.index, self.cam = index, CAMS[index]
        cam = self.cam
        self.frames = P.frames(CALIB, index)
        F = len(self.frames)
        self.member = P.masks(cam)
        self.masks = np.ascontiguousarray(np.broadcast_to(self.member, (F,) + self.member.shape))
        self.rects = LpfContext.mask_rects(self.masks)
        self.corners = P.boxes(cam, self.frames[-1])
        self.boxes = [self.corners] * F
        self._refs, self._wide = {}, None

    def ref(self, pts_index=None, f=None):
        """orc.run of frame f of this camera's batch, or of camera pts_index's full cloud, under this camera"""
        key = (pts_index, f)
        if key not in self._refs:
            pts = self.frames[f] if pts_index is None else P.cloud(CALIB, pts_index)
            cam = self.cam
            lab = orc.pack_masks(self.member, 0, cam["H"], cam["W"])
            o = orc.run(pts, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"], label_img=lab, M=3, corners=self.corners)
            vi = o["valid_idx"]
            o.update(u_valid=o["u"][vi], v_valid=o["v"][vi], label_valid=o["label_bits"][vi], n_labelled=int(np.count_nonzero(o["label_bits"])))
            self._refs[key] = o
        return self._refs[key]

    def wide_cam(self, frames):
        """the camera as wide_fuzz_cases' functions take it, with M_WIDE masks (the three, repeated) over ``frames``"""
        cam = self.cam
        mem = P.masks(cam, M_WIDE)
        return dict(T=cam["T"], K=cam["K"], W=cam["W"], H=cam["H"], dmin=cam["dmin"], dmax=cam["dmax"], M=M_WIDE, F=len(frames),
                    oriented=True, erode=0, member=[mem] * len(frames), boxes=[self.corners] * len(frames))

    def wide_refs(self):
        if self._wide is None:
            wc = self.wide_cam(self.frames)
            self._wide = [G.oracle_result(wc, p, f) for f, p in enumerate(self.frames)]
        return self._wide


def _case(index):
    if index not in _cases:
        _cases[index] = _Case(index)
    return _cases[index]


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()                          # (a copy: the shared cases are read-only)


def _same(r, o, what, keys=EXACT):
    """one frame's result in run_batch's shape against the oracle's"""
    for k in keys:
        assert np.array_equal(r[k], o[k]), (what, k)
    assert r["n_valid"] == o["n_valid"] and r["n_labelled"] == o["n_labelled"], (what, "n_valid, n_labelled")
    assert len(r["inst_lists"]) == len(o["inst_lists"]), what
    for m, (a, b) in enumerate(zip(r["inst_lists"], o["inst_lists"])):
        assert np.array_equal(a, b), (what, "inst_lists", m)
    for k in FLOATS:
        assert P.same_floats(r[k], o[k]), (what, k)


def _same_wide(r, ref, what):
    G.compare(r, ref, what)
    for k in FLOATS:
        assert P.same_floats(r[k], ref[k]), (what, k)


def _set_camera(ctx, cam):
    ctx.set_camera(cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"])


def _set_masks(ctx, c, variant, masks=None, rects=None):
    """host masks (packed), device masks lent (the direct gather), device masks lent with their rectangles (the gated direct form;
    under a large geometry the candidate grid).  Returns what must stay alive."""
    import torch
    masks = c.masks if masks is None else masks
    if variant == "host":
        ctx.set_masks(masks)
        return None
    t = _dev(masks)
    torch.cuda.synchronize()
    if variant == "lent+rects":
        ctx.set_mask_rects(c.rects if rects is None else rects)
    ctx.set_masks(t, lend=True)
    return t


# ---- run_batch, host arrays in and out ---------------------------------------------------------------------------------------------------
@INDEX
@pytest.mark.parametrize("variant", ["host", "lent", "lent+rects"])
@pytest.mark.parametrize("form", ["auto", "small-narrow", "small-1024", "large", "large-scan"])
def test_run_batch(form, variant, index):
    c = _case(index)
    with context_for_form(form) as ctx:
        _set_camera(ctx, c.cam)
        keep = _set_masks(ctx, c, variant)
        ctx.set_boxes(c.boxes)
        res = ctx.run_batch(c.frames, want_float=True, want_valid_uv=True)
        del keep
    assert len(res) == len(c.frames)
    for f, r in enumerate(res):
        _same(r, c.ref(f=f), (c.cam["name"], form, variant, f))


# ---- run_device under the software-pipelined modes --------------------------------------------------------------------------------------------
def _device_outputs(n, F, cap, M, Btot):
    import torch
    dev = torch.device("cuda", 0)
    n1 = max(n, 1)
    return dict(uv=torch.empty((n1, 2), dtype=torch.int32, device=dev), label_bits=torch.empty(n1, dtype=torch.int32, device=dev),
                depth=torch.empty(n1, dtype=torch.float64, device=dev), u_f=torch.empty(n1, dtype=torch.float64, device=dev),
                v_f=torch.empty(n1, dtype=torch.float64, device=dev), valid_idx=torch.empty(n1, dtype=torch.int64, device=dev),
                inst_idx=torch.empty((F, cap), dtype=torch.int64, device=dev), count_mb=torch.zeros(max(M * Btot, 1), dtype=torch.int32, device=dev),
                summary=torch.zeros(F * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev),
                uv_valid=torch.empty((n1, 2), dtype=torch.int32, device=dev), label_valid=torch.empty(n1, dtype=torch.int32, device=dev))


def _device_results(o, off, M, nbox):
    """device-mode outputs read back, one dict per frame in run_batch's shape (every frame has nbox boxes)"""
    h = {k: t.cpu().numpy() for k, t in o.items()}
    sm = np.frombuffer(h["summary"].tobytes(), SUMMARY_DTYPE)
    res = []
    for f in range(len(off) - 1):
        a, b = int(off[f]), int(off[f + 1])
        nv = int(sm[f]["n_valid"])
        io = sm[f]["inst_off"]
        assert int(sm[f]["inst_overflow"]) == 0
        res.append(dict(u=h["uv"][a:b, 0], v=h["uv"][a:b, 1], label_bits=h["label_bits"][a:b].view(np.uint32), depth=h["depth"][a:b],
                        uf=h["u_f"][a:b], vf=h["v_f"][a:b], valid_idx=h["valid_idx"][a:a + nv], n_valid=nv, n_labelled=int(sm[f]["n_labelled"]),
                        inst_count=sm[f]["inst_count"][:M], best_box=sm[f]["best_box"][:M], best_cnt=sm[f]["best_cnt"][:M],
                        count_mb=h["count_mb"][M * nbox * f:M * nbox * (f + 1)].reshape(M, nbox).astype(np.int64),
                        inst_lists=[h["inst_idx"][f, int(io[m]):int(io[m + 1])] for m in range(M)],
                        u_valid=h["uv_valid"][a:a + nv, 0], v_valid=h["uv_valid"][a:a + nv, 1], label_valid=h["label_valid"][a:a + nv].view(np.uint32)))
    return res


@INDEX
@pytest.mark.parametrize("form", ["auto", "large"])
@pytest.mark.parametrize("rects", [False, True], ids=["lent", "lent+rects"])
@pytest.mark.parametrize("mode", ["fused", "fused-pack"])
def test_run_device_pipelined(mode, rects, form, index):
    """Three runs with nothing synchronised between them -- the camera's own batch, then the full clouds of the next two cameras of
    the list under this camera, as one frame and as two -- so that the tail of a run rides in the launch of the next."""
    import torch
    c = _case(index)
    others = [(index + 1) % len(CAMS), (index + 2) % len(CAMS)]
    runs = [([(None, f) for f in range(len(c.frames))], c.frames),
            ([(others[0], None)], [np.array(P.cloud(CALIB, others[0]))]),
            ([(others[1], None), (None, 1)], [np.array(P.cloud(CALIB, others[1])), c.frames[1]])]
    M, nbox = 3, len(c.corners)
    held = []
    with context_for_form(form) as ctx:
        ctx.set_pipelined(mode)
        _set_camera(ctx, c.cam)
        for keys, frames in runs:
            F = len(frames)
            sizes = [len(p) for p in frames]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            cap = max(max(sizes), 1) * M
            pts = _dev(np.concatenate(frames))
            masks = np.ascontiguousarray(np.broadcast_to(c.member, (F,) + c.member.shape))
            o = _device_outputs(int(off[-1]), F, cap, M, nbox * F)
            mt = _dev(masks)
            rt = _dev(LpfContext.mask_rects(masks)) if rects else None
            torch.cuda.synchronize()
            if rects:
                ctx.set_mask_rects(rt)
            ctx.set_masks(mt, lend=True)
            ctx.set_boxes([c.corners] * F)
            ctx.run_device(pts, off, inst_cap=cap, **o)
            held.append((o, off, pts, mt, rt))
        ctx.sync()
        torch.cuda.synchronize()
        for (keys, frames), (o, off, _, _, _) in zip(runs, held):
            for f, (r, key) in enumerate(zip(_device_results(o, off, M, nbox), keys)):
                _same(r, c.ref(*key), (c.cam["name"], mode, rects, form, key))


# ---- make_frame_step: one call per frame (lpf_run_frame) -------------------------------------------------------------------------------------------
@INDEX
@pytest.mark.parametrize("rects", [False, True], ids=["masks", "masks+rects"])
@pytest.mark.parametrize("mode", ["fused", "fused-pack"])
def test_frame_step_stream(mode, rects, index):
    """three frames of a pipelined stream: E alone, the full cloud, the next camera's full cloud"""
    import torch
    c = _case(index)
    other = (index + 1) % len(CAMS)
    keys = [(None, 1), (None, 2), (other, None)]
    frames = [c.frames[1], c.frames[2], np.array(P.cloud(CALIB, other))]
    M, nbox = 3, len(c.corners)
    mt, rt = _dev(c.member), _dev(LpfContext.mask_rects(c.member))
    held = []
    with LpfContext(0) as ctx:
        ctx.set_pipelined(mode)
        _set_camera(ctx, c.cam)
        ctx.set_boxes([c.corners])
        steps = []
        for p in frames:
            n = len(p)
            o = _device_outputs(n, 1, n * M, M, nbox)
            pts = _dev(p)
            held.append((o, pts))
            steps.append(ctx.make_frame_step(pts, masks_u8=mt, mask_rects=rt if rects else None, inst_cap=n * M, **o))
        torch.cuda.synchronize()
        for s in steps:
            s()
        ctx.sync()
        torch.cuda.synchronize()
        for key, p, (o, _) in zip(keys, frames, held):
            r, = _device_results(o, np.array([0, len(p)], np.int64), M, nbox)
            _same(r, c.ref(*key), (c.cam["name"], mode, rects, key))


# ---- the wide routes -----------------------------------------------------------------------------------------------------------------------
@INDEX
@pytest.mark.parametrize("where", ["host", "device+rects"])
def test_run_wide(where, index):
    c = _case(index)
    F = len(c.frames)
    masks = np.ascontiguousarray(np.broadcast_to(P.masks(c.cam, M_WIDE), (F, M_WIDE, c.cam["H"], c.cam["W"])))
    refs = c.wide_refs()
    with LpfContext(0) as ctx:
        _set_camera(ctx, c.cam)
        ctx.set_boxes(c.boxes)
        if where == "host":
            res = ctx.run_wide(c.frames, masks, want_float=True, want_valid_uv=True)
        else:
            res = ctx.run_wide(c.frames, _dev(masks), rects=_dev(LpfContext.mask_rects(masks)), want_float=True, want_valid_uv=True)
    assert len(res) == F
    for f in range(F):
        _same_wide(res[f], refs[f], (c.cam["name"], where, f))


@INDEX
@pytest.mark.parametrize("rects", [True, False], ids=["rects", "pack"])
def test_frame_step_wide(rects, index):
    """make_frame_step_wide on the first 60 points of E (a sparse frame even on the 16 x 8 image: with rectangles it takes the direct
    form), on E and on the full cloud; which form ran is read from the context's statistics and has to be the routing rule's"""
    c = _case(index)
    E = c.frames[1]
    frames = [E[:60], E, c.frames[2]]
    wc = c.wide_cam(frames)
    mem = wc["member"][0]
    dm, dr = _dev(mem), _dev(LpfContext.mask_rects(mem))
    nbox = len(c.corners)
    seen = set()
    with LpfContext(0) as ctx:
        _set_camera(ctx, c.cam)
        ctx.set_boxes([c.corners])
        for f, p in enumerate(frames):
            ref = c.wide_refs()[f] if f else G.oracle_result(wc, p, 0)
            cap = max(int(ref["inst_count"].sum()), 1)
            o = _outs(len(p), M_WIDE, nbox, cap)
            step = ctx.make_frame_step_wide(_dev(p), dm, mask_rects=dr if rects else None, inst_cap=cap, **o)
            before = ctx.stats()["wide_direct_frames"]
            step()
            ctx.sync()
            direct = ctx.stats()["wide_direct_frames"] - before
            assert direct == int(G.expects_direct(wc, f, len(p), rects)), (c.cam["name"], f)
            seen.add(bool(direct))
            h = _host(o)
            assert h["inst_overflow"][0] == 0
            _same_wide(_frame_wide_result(h, M_WIDE, nbox), ref, (c.cam["name"], rects, f, "direct" if direct else "pack"))
    assert seen == {G.expects_direct(wc, f, len(p), rects) for f, p in enumerate(frames)}, (c.cam["name"], seen)
    if rects:
        assert True in seen, c.cam["name"]                               # every camera's sparse frame takes the direct form


# ---- the multi-camera routes: the cameras four at a time, so that different windows, sizes and K scales sit in one pass -----------------------------
GROUPS = [list(range(a, min(a + 4, len(CAMS)))) for a in range(0, len(CAMS), 4)]
GROUP = pytest.mark.parametrize("group", GROUPS, ids=lambda g: "%s..%s" % (NAMES[g[0]], NAMES[g[-1]]))


def _group_frames(group):
    """an empty frame, E, and the full cloud of every camera of the group: every camera of the pass sees them all"""
    return [np.zeros((0, 4), np.float32), np.array(P.edge_points())] + [np.array(P.cloud(CALIB, k)) for k in group]


def _spec(c, frames, M):
    cam = c.cam
    masks = np.ascontiguousarray(np.broadcast_to(P.masks(cam, M), (len(frames), M, cam["H"], cam["W"])))
    return dict(T_velo_to_rect=cam["T"], K=cam["K"], width=cam["W"], height=cam["H"], depth_min=cam["dmin"], depth_max=cam["dmax"],
                masks=masks, rects=LpfContext.mask_rects(masks), boxes=[c.corners] * len(frames), oriented=True)


@GROUP
def test_run_cams(group):
    frames = _group_frames(group)
    cases = [_case(k) for k in group]
    with LpfContext(0) as ctx:
        got = ctx.run_cams(frames, [_spec(c, frames, 3) for c in cases], want_float=True, want_valid_uv=True)
    assert len(got) == len(group)
    for c, res in zip(cases, got):
        for f, r in enumerate(res):
            key = (None, f) if f < 2 else (group[f - 2], None)
            _same(r, c.ref(*key), (c.cam["name"], "frame %d" % f))


@GROUP
def test_run_cams_wide(group):
    frames = _group_frames(group)
    cases = [_case(k) for k in group]
    with LpfContext(0) as ctx:
        got = ctx.run_cams_wide(frames, [_spec(c, frames, M_WIDE) for c in cases], want_float=True, want_valid_uv=True)
    assert len(got) == len(group)
    for c, res in zip(cases, got):
        wc = c.wide_cam(frames)
        for f, r in enumerate(res):
            _same_wide(r, G.oracle_result(wc, frames[f], f), (c.cam["name"], "frame %d" % f))


# ---- the depth routes --------------------------------------------------------------------------------------------------------------------------
@INDEX
def test_depth_image_and_depth_maps(index):
    c = _case(index)
    cam = c.cam
    want = [orc.depth_image(p, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"]) for p in c.frames]
    with LpfContext(0) as ctx:
        _set_camera(ctx, cam)
        got = [ctx.depth_image(p) for p in c.frames]
        maps = ctx.depth_maps(c.frames, c.masks, binarize="astype")
        maps_r = ctx.depth_maps(c.frames, _dev(c.masks), binarize="astype", rects=_dev(c.rects), cap=1)
    for f, ((D, win), (wD, wwin)) in enumerate(zip(got, want)):
        assert np.array_equal(win, wwin), (cam["name"], f, "winner")
        assert np.array_equal(P.bits(D), P.bits(wD)), (cam["name"], f, "D")               # (a valid point's depth is no NaN)
        cars = _expect(wD, wwin, c.member.astype(bool))
        _same_maps(maps[f], cars, (cam["name"], f))
        _same_maps(maps_r[f], cars, (cam["name"], f, "device masks, rectangles, cap=1"))
    if cam["dmin"] < -1e-6 and cam["kind"] == "ties":
        # the valid d == 0 point that wins its pixel shows the substituted depth there
        pts, (D, win), (wD, wwin) = c.frames[2], got[2], want[2]
        o = c.ref(f=2)
        d0 = [i for i in o["valid_idx"] if o["depth"][i] == -1e-6 and wwin[o["v"][i], o["u"][i]] == i]
        assert d0, cam["name"]
        for i in d0:
            assert D[o["v"][i], o["u"][i]] == -1e-6 and win[o["v"][i], o["u"][i]] == i


# ---- the box routes, on the cam-0 corner sets ------------------------------------------------------------------------------------------------------
def _box_reference(e):
    corners, names = P.box_corner_sets()
    K = P.box_K(e)
    Tvc = np.asarray(CALIB["TrVeloToCam"], np.float64)
    Tcv = np.linalg.inv(Tvc)
    off = np.array([0, 7, 7, len(corners)], np.int32)                        # three frames, the middle one without a box
    ref = bv.views(corners, off, K, P.BOX_W, P.BOX_H, Tcv, want=bv.WANT)
    visible, _ = npp.prepare_boxes(corners, K, P.BOX_W, P.BOX_H, Tvc)
    return np.array(corners), names, K, Tcv, off, ref, visible


def _same_boxes(got, ref, visible, names, what):
    vis, cv, bb, fr = got
    bad = lambda a, b: [n for n, x, y in zip(names, a, b) if not bv.same_bits(np.asarray(x), np.asarray(y))]
    assert np.array_equal(np.asarray(vis).astype(bool), visible), (what, "visible", bad(np.asarray(vis).astype(bool), visible))
    assert np.array_equal(fr, ref["front"]), (what, "front", bad(fr, ref["front"]))
    assert bv.same_bits(bb, ref["bbox2d"]), (what, "bbox2d", bad(bb, ref["bbox2d"]))
    assert bv.same_bits(cv, ref["corners_velo"]), (what, "corners_velo", bad(cv, ref["corners_velo"]))


@pytest.mark.parametrize("e", P.BOX_SCALES)
def test_box_routes(e):
    """prepare_boxes, set_boxes_cam0 in a serial context, set_boxes_cam0 in a pipelined context (the box job rides in the next run's
    launch) and box_views: visible, front, bbox2d and corners_velo bit for bit against tests/box_views_ref.py, and so with each other"""
    import torch
    corners, names, K, Tcv, off, ref, visible = _box_reference(e)
    B = len(corners)
    per_frame = [corners[a:b] for a, b in zip(off[:-1], off[1:])]
    E = np.array(P.edge_points())
    with LpfContext(0) as ctx:
        ctx.set_camera(np.eye(4), K, P.BOX_W, P.BOX_H, 0.0, 50.0)
        _same_boxes(ctx.prepare_boxes(corners, Tcv), ref, visible, names, "prepare_boxes")
        out = ctx.set_boxes_cam0(per_frame, Tcv, want_outputs=True)
        cat = [np.concatenate([o[k] for o in out]) for k in range(4)]
        _same_boxes(cat, ref, visible, names, "set_boxes_cam0, serial")
        v = ctx.box_views(corners, off, Tcv, want=("front", "bbox2d", "near_bbox2d", "corners_near", "corners_in_view", "corners_velo"))
        for k in ("front", "corners_near", "corners_in_view"):
            assert np.array_equal(v[k], ref[k]), ("box_views", k)
        for k in ("bbox2d", "near_bbox2d", "corners_velo"):
            assert bv.same_bits(v[k], ref[k]), ("box_views", k)
    dev = torch.device("cuda", 0)
    F = len(off) - 1
    o = dict(visible=torch.zeros(B, dtype=torch.uint8, device=dev), corners_velo=torch.zeros((B, 8, 3), dtype=torch.float64, device=dev),
             bbox2d=torch.zeros((B, 4), dtype=torch.float64, device=dev), front=torch.zeros(B, dtype=torch.int32, device=dev))
    pts = _dev(np.concatenate([E] * F))
    poff = np.arange(F + 1, dtype=np.int64) * len(E)
    ro = _device_outputs(len(E) * F, F, 1, 0, B)
    dc = _dev(corners)
    torch.cuda.synchronize()
    with LpfContext(0) as ctx:
        ctx.set_pipelined("fused")
        ctx.set_camera(np.eye(4), K, P.BOX_W, P.BOX_H, 0.0, 50.0)
        ctx.clear_masks()
        ctx.set_boxes_cam0_device(dc, off, Tcv, lend=True, **o)
        ctx.run_device(pts, poff, uv=ro["uv"], valid_idx=ro["valid_idx"], count_mb=ro["count_mb"], summary=ro["summary"])
        st = ctx.stats()
        ctx.sync()
    torch.cuda.synchronize()
    assert st["box_jobs_riding"] == 1 and st["box_jobs_alone"] == 0, st
    _same_boxes([o[k].cpu().numpy() for k in ("visible", "corners_velo", "bbox2d", "front")], ref, visible, names, "set_boxes_cam0, pipelined")
    want = orc.run(E, np.eye(4), K, P.BOX_W, P.BOX_H, 0.0, 50.0, want_float=False)
    uv = ro["uv"].cpu().numpy()
    assert np.array_equal(uv[:len(E), 0], want["u"]) and np.array_equal(uv[:len(E), 1], want["v"])
