"""lpf_run_wide / LpfContext.run_wide on the GPU: frames with up to 256 masks in one native pass, against the pinned C oracle run
once per group of 32 masks (label word w = group w), and against the narrow path for the float outputs."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, unpack_masks
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd._native import LpfContext, LpfError, WideInput, WideOutputs
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cal(calib):
    _, T, K, W, H = S.default_calibration(calib)
    return dict(T=T, K=K, W=W, H=H, calib=calib)


@pytest.fixture(scope="module")
def ctx(cal):
    c = LpfContext(0)
    c.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, 50.0)
    yield c
    c.close()


def _masks(M, seed, W, H):
    """M disk masks that overlap (the same disk several times) with some empty ones among them."""
    m, _ = S.synthetic_disk_masks(M, seed, W, H)
    rng = np.random.default_rng(seed)
    for i in rng.choice(M, size=M // 7, replace=False):
        m[i] = 0
    if M > 3:
        m[M // 2] = m[1]
    return m, LpfContext.mask_rects(m)


def _boxes(B, seed, calib):
    if B == 0:
        return np.zeros((0, 8, 3))
    return S.synthetic_boxes(B, seed, np.asarray(calib["TrVeloToCam"]))[1]


def _check(cal, res, pts_list, member, erode, corners, oriented, inst_full=True, dmin=0.0, dmax=50.0):
    """res: run_wide's list; member: per frame uint8 [M,H,W] (the binarised masks, before erosion); dmin, dmax: the camera's depth window."""
    W, H = cal["W"], cal["H"]
    for f, (r, pts, mem, cor) in enumerate(zip(res, pts_list, member, corners)):
        M = mem.shape[0]
        LW = (M + 31) // 32
        assert r["label_words"].shape == (len(pts), LW)
        assert len(r["inst_count"]) == M and len(r["best_box"]) == M and r["count_mb"].shape == (M, len(cor))
        if len(pts) == 0:
            assert r["n_valid"] == 0 and r["n_labelled"] == 0 and all(len(l) == 0 for l in r["inst_lists"])
            assert not r["inst_count"].any() and (r["best_box"] == -1).all()
            continue
        anyw = np.zeros(len(pts), bool)
        for w in range(LW):
            grp = mem[32 * w:32 * w + 32]
            o = orc.run(pts, cal["T"], cal["K"], W, H, dmin, dmax, label_img=orc.pack_masks(grp, erode, H, W), M=len(grp),
                        corners=cor, oriented=oriented, want_float=False)
            assert np.array_equal(r["label_words"][:, w], o["label_bits"]), "word %d" % w
            assert np.array_equal(r["u"], o["u"]) and np.array_equal(r["v"], o["v"])
            assert np.array_equal(r["valid_idx"], o["valid_idx"])
            assert np.array_equal(r["count_mb"][32 * w:32 * w + len(grp)], o["count_mb"]), "count_mb word %d" % w
            assert np.array_equal(r["best_box"][32 * w:32 * w + len(grp)], o["best_box"])
            assert np.array_equal(r["best_cnt"][32 * w:32 * w + len(grp)], o["best_cnt"])
            assert np.array_equal(r["inst_count"][32 * w:32 * w + len(grp)], o["inst_count"])
            for m in range(len(grp)):
                assert np.array_equal(r["inst_lists"][32 * w + m], o["inst_lists"][m]), "list %d" % (32 * w + m)
            anyw |= o["label_bits"] != 0
        assert r["n_valid"] == len(r["valid_idx"]) and r["n_labelled"] == int(anyw.sum())
        if "label_valid_words" in r:
            assert np.array_equal(r["label_valid_words"], r["label_words"][r["valid_idx"]])
            assert np.array_equal(r["u_valid"], r["u"][r["valid_idx"]]) and np.array_equal(r["v_valid"], r["v"][r["valid_idx"]])


@pytest.mark.parametrize("M", [1, 32, 33, 64, 100, 256])
def test_wide_uint8_host_masks(ctx, cal, M):
    sc = S.scene(60_000, n_masks=1, n_boxes=1, seed=M, calib=cal["calib"])
    masks, _ = _masks(M, 11 + M, cal["W"], cal["H"])
    cor = _boxes(7, M, cal["calib"])
    ctx.set_boxes([cor], oriented=True)
    res = ctx.run_wide([sc["points"]], masks, want_valid_uv=True)
    _check(cal, res, [sc["points"]], [masks], 0, [cor], True)


def test_wide_float_outputs_equal_the_narrow_path(ctx, cal):
    sc = S.scene(50_000, n_masks=1, n_boxes=1, seed=5, calib=cal["calib"])
    masks, _ = _masks(40, 5, cal["W"], cal["H"])
    ctx.set_boxes([_boxes(7, 5, cal["calib"])], oriented=True)
    rw = ctx.run_wide([sc["points"]], masks, want_float=True)[0]
    ctx.set_masks(masks[:32])
    rn = ctx.run_batch([sc["points"]], want_float=True)[0]
    for k in ("depth", "uf", "vf"):
        assert np.array_equal(rw[k].view(np.uint64), rn[k].view(np.uint64)), k
    assert np.array_equal(rw["label_words"][:, 0], rn["label_bits"])


@pytest.mark.parametrize("binarize,erode", [("astype", 0), ("astype", 1), ("v3", 1), ("v3", 2), ("gt0.5", 0), ("gt0.5", 2)])
def test_wide_float_masks_binarize_and_erosion(ctx, cal, binarize, erode):
    sc = S.scene(40_000, n_masks=1, n_boxes=1, seed=9, calib=cal["calib"])
    u8, _ = _masks(70, 9, cal["W"], cal["H"])
    rng = np.random.default_rng(3)
    fm = u8.astype(np.float32) * rng.choice(np.array([0.3, 0.6, 1.0, 2.5], np.float32), size=(70, 1, 1))   # values each rule treats apart
    if binarize == "astype":
        member = orc.binarize_f32(fm, False)
    elif binarize == "v3":
        member = orc.binarize_f32(fm, True)
    else:
        member = (fm > 0.5).astype(np.uint8)
    cor = _boxes(7, 9, cal["calib"])
    ctx.set_boxes([cor], oriented=True)
    res = ctx.run_wide([sc["points"]], fm, erode_iters=erode, binarize=binarize)
    _check(cal, res, [sc["points"]], [member], erode, [cor], True)


@pytest.mark.parametrize("f32", [False, True])
def test_wide_device_masks_with_rects(ctx, cal, f32):
    import torch
    sc = S.scene(50_000, n_masks=1, n_boxes=1, seed=21, calib=cal["calib"])
    masks, rects = _masks(64, 21, cal["W"], cal["H"])
    cor = _boxes(65, 21, cal["calib"])
    ctx.set_boxes([cor], oriented=True)
    dm = torch.from_numpy(masks.astype(np.float32) if f32 else masks).cuda()
    dr = torch.from_numpy(rects[None].copy()).cuda()
    res = ctx.run_wide([sc["points"]], dm, rects=dr, want_valid_uv=True)
    _check(cal, res, [sc["points"]], [masks], 0, [cor], True)
    # host masks, host rectangles, device points
    res = ctx.run_wide([torch.from_numpy(sc["points"]).cuda()], masks, rects=rects)
    _check(cal, res, [sc["points"]], [masks], 0, [cor], True)


@pytest.mark.parametrize("oriented", [True, False])
def test_wide_three_frames_unequal(ctx, cal, oriented):
    sizes = [30_000, 0, 45_000]
    pts = [S.scene(n, n_masks=1, n_boxes=1, seed=40 + i, calib=cal["calib"])["points"] if n else np.zeros((0, 4), np.float32)
           for i, n in enumerate(sizes)]
    mk = np.stack([_masks(100, 50 + i, cal["W"], cal["H"])[0] for i in range(3)])
    cor = [_boxes(b, 60 + i, cal["calib"]) for i, b in enumerate((7, 0, 65))]
    ctx.set_boxes(cor, oriented=oriented)
    res = ctx.run_wide(pts, mk, want_valid_uv=True)
    _check(cal, res, pts, list(mk), 0, cor, oriented)
    ctx.set_boxes([np.zeros((0, 8, 3))] * 3, oriented=oriented)      # B = 0 everywhere
    res = ctx.run_wide(pts, mk)
    _check(cal, res, pts, list(mk), 0, [np.zeros((0, 8, 3))] * 3, oriented)


@pytest.mark.parametrize("M", [40, 200])
def test_wide_golden_frame_100(ctx, cal, M):
    g = load_golden(100)
    W, H = cal["W"], cal["H"]
    base = unpack_masks(g, "rect5", H, W).astype(np.uint8)
    tiles = [np.roll(base[i % len(base)], shift=(7 * (i // len(base))) % W, axis=1) for i in range(M)]
    mk = np.stack(tiles)
    cor = np.asarray(g["corners_velo"])
    for oriented in (True, False):
        ctx.set_boxes([cor], oriented=oriented)
        res = ctx.run_wide([g["points"]], mk, want_valid_uv=True)
        _check(cal, res, [g["points"]], [mk], 0, [cor], oriented)


def test_wide_agrees_with_the_numpy_path(ctx, cal):
    sc = S.scene(40_000, n_masks=1, n_boxes=1, seed=77, calib=cal["calib"])
    masks, _ = _masks(100, 77, cal["W"], cal["H"])
    cor = _boxes(12, 77, cal["calib"])
    ctx.set_boxes([cor], oriented=True)
    r = ctx.run_wide([sc["points"]], masks)[0]
    K3 = np.asarray(cal["K"]).reshape(3, 3)
    u, v, vi, lists, count, best_box, best_cnt = npp.frame_path(sc["points"], np.asarray(cal["T"]).reshape(4, 4), K3, cal["W"], cal["H"],
                                                                  50.0, masks, cor)
    assert np.array_equal(r["valid_idx"], vi)
    for m in range(100):
        assert np.array_equal(r["inst_lists"][m], lists[m])
    assert np.array_equal(r["count_mb"], count) and np.array_equal(r["best_box"], best_box) and np.array_equal(r["best_cnt"], best_cnt)


# ---- errors and state ------------------------------------------------------------------------------------------------------------
def _raw_wide(ctx, pts, M, masks=None):
    off = np.array([0, len(pts)], np.int64)
    inp = WideInput(masks=masks.ctypes.data if masks is not None else None, M=M, f32=0, binarize=0, erode_iters=0, on_device=0)
    n_valid = np.zeros(1, np.int64)
    out = WideOutputs(n_valid=n_valid.ctypes.data, on_device=0)
    return ctx._lib.lpf_run_wide(ctx._h, pts.ctypes.data, off.ctypes.data, 1, 0, ctypes.byref(inp), ctypes.byref(out)), n_valid


def test_wide_refuses_257_and_negative(ctx, cal):
    pts = S.scene(1000, n_masks=1, n_boxes=1, seed=1, calib=cal["calib"])["points"]
    mk = np.zeros((257, cal["H"], cal["W"]), np.uint8)
    assert _raw_wide(ctx, pts, 257, mk)[0] == -1
    assert _raw_wide(ctx, pts, -1, mk)[0] == -1
    rc, nv = _raw_wide(ctx, pts, 256, mk[:256])
    assert rc == 0 and nv[0] > 0


def test_wide_is_refused_inside_graph_capture(cal):
    pts = S.scene(2000, n_masks=1, n_boxes=1, seed=2, calib=cal["calib"])["points"]
    with LpfContext(0) as c:
        c.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, 50.0)
        c.graph_begin()
        rc, _ = _raw_wide(c, pts, 40, np.zeros((40, cal["H"], cal["W"]), np.uint8))
        assert rc == -3                                                         # LPF_ERR_STATE
        try:
            c.graph_end()
        except LpfError:
            pass


def test_narrow_calls_still_refuse_33(ctx, cal):
    with pytest.raises(LpfError):
        ctx.set_masks(np.zeros((33, cal["H"], cal["W"]), np.uint8))


def test_wide_between_pipelined_narrow_runs(cal):
    import torch
    sc = S.scene(60_000, n_masks=5, n_boxes=9, seed=31, calib=cal["calib"])
    W, H = cal["W"], cal["H"]
    big, _ = _masks(50, 31, W, H)
    with LpfContext(0) as c:
        c.set_camera(cal["T"], cal["K"], W, H, 0.0, 50.0)
        c.set_pipelined(4)
        dev = torch.device("cuda", 0)
        pts = torch.from_numpy(sc["points"]).to(dev)
        n = len(sc["points"])
        outs = []
        for step in range(2):
            c.set_masks(torch.from_numpy(sc["masks"]).to(dev), lend=True)
            c.set_boxes([sc["corners_velo"]])
            uv = torch.empty((n, 2), dtype=torch.int32, device=dev)
            lab = torch.empty(n, dtype=torch.int32, device=dev)
            vidx = torch.empty(n, dtype=torch.int64, device=dev)
            c.run_device(pts, np.array([0, n], np.int64), uv=uv, label_bits=lab, valid_idx=vidx)
            outs.append((uv, lab, vidx))
            if step == 0:                                   # the wide call between the two narrow runs
                rw = c.run_wide([sc["points"]], big)
                _check(cal, rw, [sc["points"]], [big], 0, [sc["corners_velo"]], True)
        c.sync()
        o = orc.run(sc["points"], cal["T"], cal["K"], W, H, 0.0, 50.0, label_img=orc.pack_masks(sc["masks"], 0, H, W), M=5,
                    corners=sc["corners_velo"], want_float=False)
        for uv, lab, vidx in outs:
            assert np.array_equal(uv.cpu().numpy()[:, 0], o["u"]) and np.array_equal(uv.cpu().numpy()[:, 1], o["v"])
            assert np.array_equal(lab.cpu().numpy().view(np.uint32), o["label_bits"])
            assert np.array_equal(vidx.cpu().numpy()[:o["n_valid"]], o["valid_idx"])


# ---- the Python pipeline: the wide pass equals the per-group passes ----------------------------------------------------------------
def _camera(calib):
    return kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))


def _same(a, b):
    assert np.array_equal(a["valid_indices"], b["valid_indices"])
    assert np.array_equal(a["count_mb"], b["count_mb"])
    assert np.array_equal(a["bg_assigned"], b["bg_assigned"])
    assert len(a["car_point_sets"]) == len(b["car_point_sets"])
    for x, y in zip(a["car_point_sets"], b["car_point_sets"]):
        assert np.array_equal(x, y)
    assert a["car_statistics"] == b["car_statistics"]


@pytest.mark.parametrize("M,erode,f32,scan", [(40, 0, True, False), (100, 1, False, False), (300, 0, False, False), (100, 1, False, True)],
                         ids=["40-0-True", "100-1-False", "300-0-False", "100-1-False-scan"])
def test_run_frames_wide_equals_mask_groups(cal, M, erode, f32, scan, tmp_path):
    calib = cal["calib"]
    cam = _camera(calib)
    frames = []
    for i, n in enumerate((40_000, 25_000)):
        sc = S.scene(n, n_masks=1, n_boxes=12, seed=90 + i, calib=calib)
        mk, _ = _masks(M - 3 * i, 90 + i, cal["W"], cal["H"])
        mk = mk.astype(np.float32) if f32 else mk
        boxes = [{"corners_velo": c.tolist()} for c in sc["corners_velo"]]
        colors = [(i, j % 255, 0) for j in range(M)]
        frames.append(pipeline.FrameInputs(i, sc["points"], mk, boxes, colors))
    ctx = pipeline.get_context(0)
    if scan:                                     # the scans through the read-ahead reader: the wide pass reads each Scan where it is
        paths = [tmp_path / ("%010d.bin" % f.frame) for f in frames]
        for f, p in zip(frames, paths):
            f.points.tofile(p)
        inputs = lambda i, path: (frames[i].frame, frames[i].masks, frames[i].bboxes_3d, frames[i].colors)     # noqa: E731
        r_wide = list(pipeline.stream_frames(paths, inputs, calib["TrVeloToRect"], cam, 50.0, 10, True, erode_iters=erode))
    else:
        r_wide = pipeline.run_frames(frames, calib["TrVeloToRect"], cam, 50.0, 10, True, erode_iters=erode)
    assert len(r_wide) == len(frames)
    stacks = [pipeline._mask_stack(f.masks, cam, resize_ctx=ctx)[0] for f in frames]
    r_grp = pipeline._run_frames_in_mask_groups(frames, stacks, calib["TrVeloToRect"], cam, 50.0, 10, True, erode, False, 0, ctx)
    for a, b in zip(r_wide, r_grp):
        _same(a, b)


def test_extract_car_points_by_mask_wide(cal):
    calib = cal["calib"]
    cam = _camera(calib)
    g = load_golden(100)
    base = unpack_masks(g, "rect5", cam.height, cam.width)
    masks = [np.roll(base[i % 5], 5 * (i // 5), axis=0) for i in range(45)]
    vi = g["valid_idx_d50"]
    pv, uv, vv = g["points"][vi, :3], g["u"][vi], g["v"][vi]
    sets = pipeline.extract_car_points_by_mask(pv, uv, vv, masks, cam)
    assert len(sets) == 45
    for m, s in enumerate(sets):
        sel = masks[m].astype(np.uint8)[vv, uv] > 0.5
        assert np.array_equal(s, pv[sel] if sel.any() else np.array([]).reshape(0, 3))
