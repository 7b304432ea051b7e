"""lpf_depth_maps / LpfContext.depth_maps / depth_maps_frames / process_frames_depth_maps on the GPU: seg_with_pointcloud's per-car
depth maps as sparse lists.  Car m of a frame must be np.flatnonzero(np.where(member_m, D, 0)) with D the last-writer depth image,
bit for bit -- against the reference-generated golden lists, the C oracle's depth image and winners, per_car_depth_maps, and
lpf_run_wide's label words for every mask rule."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_frames, load_golden, unpack_masks
from lidar_object_detection_amd import pipeline
from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd._native import SUMMARY_DTYPE, DepthMapsOutputs, LpfContext, ScanReader, WideInput
from oracle import cpu_oracle as orc

pytestmark = pytest.mark.gpu

FULL = (1461, 2098, 2449)
DMAX = 30.0


@pytest.fixture(scope="module")
def cal(calib):
    return dict(T=np.asarray(calib["TrVeloToRect"], np.float64), K=np.asarray(calib["K"], np.float64)[:3, :3], W=int(calib["width"]),
                H=int(calib["height"]), calib=calib)


@pytest.fixture(scope="module")
def gold(cal):
    """frame -> dict(pts, rect5, edge) for the 20 sample frames and the 3 full-size ones (masks uint8 [M,H,W]; frame 2717 has none)"""
    out = {}
    H, W = cal["H"], cal["W"]
    for r in golden_frames()["frames"]:
        g = load_golden(r["frame"])
        d = dict(pts=np.ascontiguousarray(g["points"], np.float32))
        for kind in ("rect5", "edge"):
            key = "masks_%s_packed" % kind
            d[kind] = unpack_masks(g, kind, H, W).astype(np.uint8) if key in g else np.zeros((0, H, W), np.uint8)
        out[r["frame"]] = d
    for f in FULL:
        g = dict(np.load(os.path.join(GOLDEN, "frame_%010d_full.npz" % f)))
        out[("full", f)] = dict(pts=np.ascontiguousarray(g["points"], np.float32), rect5=unpack_masks(g, "rect5", H, W).astype(np.uint8),
                                edge=unpack_masks(g, "edge", H, W).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def ctx(cal):
    c = LpfContext(0)
    c.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, DMAX)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle(cal, pts):
    return orc.depth_image(pts, cal["T"], cal["K"], cal["W"], cal["H"], 0.0, DMAX)


def _expect(D, win, member):
    """car lists of the definition: flatnonzero(where(member_m, D, 0)), D there, the winners there"""
    out = []
    for m in member:
        p = np.flatnonzero(np.where(m, D, 0.0))
        out.append((p, D.ravel()[p], win.ravel()[p].astype(np.int64)))
    return out


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for m, ((gp, gd, gi), (wp, wd, wi)) in enumerate(zip(got, want)):
        assert np.array_equal(gp, wp), (what, m, len(gp), len(wp))
        assert np.array_equal(np.asarray(gd).view(np.int64), np.asarray(wd).view(np.int64)), (what, m)
        if wi is not None and gi is not None:
            assert np.array_equal(gi, wi), (what, m)


def _rects(masks, pad=0, W=None, H=None):
    r = LpfContext.mask_rects(masks).astype(np.int64)
    if pad:
        r[:, :2] = np.maximum(r[:, :2] - pad, 0)
        r[:, 2] = np.minimum(r[:, 2] + pad, W)
        r[:, 3] = np.minimum(r[:, 3] + pad, H)
    return np.ascontiguousarray(r, np.int32)


class _Cam:
    def __init__(self, cal):
        self.width, self.height, self.K = cal["W"], cal["H"], cal["K"]


# ---- 1. frame 100 against the reference-generated lists ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["u8-host", "u8-dev", "f32-host", "f32-dev"])
def test_frame100_equals_the_reference_lists(ctx, gold, form):
    g = np.load(os.path.join(GOLDEN, "frame_0000000100.npz"))
    idx, val, off = g["depthmap_idx_rect5"], g["depthmap_val_rect5"], g["depthmap_off_rect5"]
    fr = gold[100]
    masks = fr["rect5"] if form.startswith("u8") else fr["rect5"].astype(np.float32)
    pts = fr["pts"]
    if form.endswith("dev"):
        masks, pts = _dev(masks), _dev(pts)
    res = ctx.depth_maps([pts], masks, binarize="gt0.5")[0]
    want = [(idx[off[m]:off[m + 1]], val[off[m]:off[m + 1]], None) for m in range(5)]
    _same(res, want, form)


def test_raw_call_host_and_device_outputs_agree(ctx, gold):
    """the C call with device outputs (lent GPU buffers, enqueue only) gives what the host outputs give: pix, depth, car_off"""
    import torch
    fr = gold[100]
    n, M, cap = len(fr["pts"]), 5, 20000
    dp, dm = _dev(fr["pts"]), _dev(fr["rect5"])
    o = {k: torch.full(s, -7, dtype=getattr(torch, t), device="cuda") for k, s, t in
         (("pix", (cap,), "int64"), ("depth", (cap,), "float64"), ("point_idx", (cap,), "int64"), ("car_off", (M + 1,), "int64"),
          ("need", (1,), "int64"), ("overflow", (1,), "int32"))}
    out = DepthMapsOutputs()
    for k, t in o.items():
        setattr(out, k, t.data_ptr())
    out.cap, out.on_device = cap, 1
    inp = WideInput()
    inp.masks, inp.M, inp.on_device = dm.data_ptr(), M, 1
    off = np.array([0, n], np.int64)
    ctx._check(ctx._lib.lpf_depth_maps(ctx._h, dp.data_ptr(), off.ctypes.data, 1, 1, ctypes.byref(inp), ctypes.byref(out)))
    ctx.sync()
    h = {k: t.cpu().numpy() for k, t in o.items()}
    g = np.load(os.path.join(GOLDEN, "frame_0000000100.npz"))
    assert np.array_equal(h["car_off"], g["depthmap_off_rect5"])
    assert h["need"][0] == 8359 and h["overflow"][0] == 0
    assert np.array_equal(h["pix"][:8359], g["depthmap_idx_rect5"])
    assert np.array_equal(h["depth"][:8359].view(np.int64), g["depthmap_val_rect5"].view(np.int64))
    assert (h["pix"][8359:] == -7).all()                        # nothing beyond need is written
    host = ctx.depth_maps([fr["pts"]], fr["rect5"])[0]
    assert np.array_equal(np.concatenate([c[2] for c in host]), h["point_idx"][:8359])


# ---- 2. all golden frames in one call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rect5", "edge"])
def test_all_golden_frames_in_one_call(ctx, cal, gold, kind):
    keys = [k for k in gold if not isinstance(k, tuple)] + [("full", f) for f in FULL]
    frames = [pipeline.FrameInputs(k if not isinstance(k, tuple) else k[1], gold[k]["pts"], gold[k][kind]) for k in keys]
    assert len(frames) == 23 and len({len(f.masks) for f in frames}) > 1           # M differs per frame
    cam = _Cam(cal)
    res = pipeline.depth_maps_frames(frames, cal["T"], cam, DMAX, ctx=ctx)
    for k, f, cars in zip(keys, frames, res):
        D, win = _oracle(cal, f.points)
        want = _expect(D, win, [m > 0.5 for m in f.masks])
        assert [c for c, _ in cars] == list(range(1, len(f.masks) + 1))
        _same([(s.pixels, s.depth, s.point_idx) for _, s in cars], want, (kind, k))
    for k, f, cars in zip(keys, frames, res):                  # the yardstick, frame by frame (it changes the shared context's camera)
        ref = pipeline.per_car_depth_maps(f.points, cal["T"], cam, f.masks.astype(np.float32), DMAX)
        for (cid, s), (rid, dense) in zip(cars, ref):
            assert cid == rid
            assert np.array_equal(s.to_dense().view(np.int64), dense.view(np.int64)), (kind, k, cid)
    ctx.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, DMAX)


# ---- 3. many points per pixel: the last writer wins --------------------------------------------------------------------------------
def test_last_writer_wins_on_a_dense_cloud(ctx, cal):
    pts = S.synthetic_cloud(3_000_000, seed=9)
    D, win = _oracle(cal, pts)
    masks, _ = S.synthetic_disk_masks(12, 9, cal["W"], cal["H"])
    masks = masks.astype(np.uint8)
    masks[0] = 1                                                # a full-image mask: every winner
    res = ctx.depth_maps([pts], masks, binarize="astype")[0]
    _same(res, _expect(D, win, masks != 0), "dense")
    assert len(res[0][0]) == int((win >= 0).sum())


# ---- 4. mask counts, rectangles and every mask rule against lpf_run_wide's label words ------------------------------------------
def _mask_set(gold, M, seed, W, H, tiled):
    if M == 0:
        return np.zeros((0, H, W), np.uint8)
    if tiled:
        m5 = gold[100]["rect5"]
        m = np.stack([np.roll(m5[i % 5], 41 * (i // 5), axis=1) for i in range(M)])
    else:
        m, _ = S.synthetic_disk_masks(M, seed, W, H)
        m = m.astype(np.uint8)
    m[3::7] = 0
    return np.ascontiguousarray(m)


def _from_words(pts, cal, words, M):
    """car lists from run_wide's label_words: the frame's winning points whose bit m is set, by pixel"""
    D, win = _oracle(cal, pts)
    wf = win.ravel()
    pix = np.flatnonzero(wf >= 0)
    wp = wf[pix]
    out = []
    for m in range(M):
        sel = ((words[wp, m // 32] >> np.uint32(m % 32)) & 1).astype(bool)
        p = pix[sel]
        out.append((p, D.ravel()[p], wf[p].astype(np.int64)))
    return out


@pytest.mark.parametrize("M", [0, 1, 32, 33, 64, 256])
@pytest.mark.parametrize("tiled", [True, False])
def test_mask_counts_and_rectangles(ctx, cal, gold, M, tiled):
    W, H = cal["W"], cal["H"]
    pts = gold[("full", 2098)]["pts"] if tiled else gold[100]["pts"]
    masks = _mask_set(gold, M, 5 + M, W, H, tiled)
    base = ctx.depth_maps([pts], masks, binarize="astype")[0]
    assert len(base) == M
    if M:
        D, win = _oracle(cal, pts)
        _same(base, _expect(D, win, masks != 0), ("plain", M))
        for pad in (0, 9):
            _same(ctx.depth_maps([pts], masks, binarize="astype", rects=_rects(masks, pad, W, H))[0], base, ("rects", M, pad))
            _same(ctx.depth_maps([pts], _dev(masks), binarize="astype", rects=_dev(_rects(masks, pad, W, H)))[0], base, ("dev rects", M, pad))


def test_host_masks_of_more_than_one_chunk(ctx, cal, gold):
    """Eight sample frames with 64 host uint8 masks and their rectangles each, just over what one chunk stages: a frame costs
    4 hwp + 12 M ntile + M (W H + 16) + 16 max N bytes of scratch (lpf_depth_maps), 38 MB here, so seven frames fit the 256 MiB of a
    chunk and the eighth is a chunk of its own -- its points, masks and rectangles are staged from an offset, its lists land behind
    the first chunk's.  Every list against the definition, bit for bit.  The split itself is not observed at run time: the assert
    below restates the host's cost formula and has to follow it (a kernel trace of this case shows lpf_dm_frame once per chunk)."""
    W, H, M = cal["W"], cal["H"], 64
    keys = sorted(k for k in gold if not isinstance(k, tuple))[:8]
    pts = [gold[k]["pts"] for k in keys]
    ntile = (W * H + 1023) // 1024
    per_frame = 4 * ntile * 1024 + 12 * M * ntile + M * (W * H + 16) + 16 * max(len(p) for p in pts)
    assert 7 * per_frame <= (256 << 20) < 8 * per_frame
    base = _mask_set(gold, M, 0, W, H, True)
    masks = np.stack([np.roll(base, 29 * f, axis=2) for f in range(len(keys))])     # another set per frame
    rects = np.stack([_rects(m) for m in masks])
    res = ctx.depth_maps(pts, masks, binarize="astype", rects=rects)
    assert len(res) == len(keys)
    for f, k in enumerate(keys):
        D, win = _oracle(cal, pts[f])
        _same(res[f], _expect(D, win, masks[f] != 0), ("chunks", k))
    assert sum(len(c[0]) for c in res[7]) > 1000                # the second chunk found its points


@pytest.mark.parametrize("rule", ["u8", "astype", "v3", "gt0.5"])
@pytest.mark.parametrize("erode", [0, 1])
@pytest.mark.parametrize("M", [5, 40])
def test_every_mask_rule_against_run_wide(ctx, cal, gold, rule, erode, M):
    W, H = cal["W"], cal["H"]
    pts = gold[100]["pts"]
    u8 = _mask_set(gold, M, 11, W, H, True)
    rng = np.random.default_rng(M + erode)
    masks = u8 if rule == "u8" else (u8 * rng.choice(np.array([0.3, 0.7, 1.0], np.float32), size=u8.shape)).astype(np.float32)
    binarize = "astype" if rule == "u8" else rule
    got = ctx.depth_maps([pts], masks, binarize=binarize, erode_iters=erode)[0]
    r = ctx.run_wide([pts], masks, erode_iters=erode, binarize=binarize, want_lists=False)[0]
    _same(got, _from_words(pts, cal, r["label_words"], M), (rule, erode, M))


# ---- 5. edge cases ----------------------------------------------------------------------------------------------------------------
def test_edge_cases(ctx, cal, gold):
    W, H = cal["W"], cal["H"]
    m5 = gold[100]["rect5"]
    empty = np.zeros((0, 4), np.float32)
    far = gold[100]["pts"].copy()
    far[:, :3] *= 100.0                                         # every point beyond the window (or behind the camera)
    res = ctx.depth_maps([empty, far, gold[100]["pts"]], np.stack([m5, m5, m5]))
    assert all(len(p) == 0 for p, _, _ in res[0]) and all(len(p) == 0 for p, _, _ in res[1])
    assert sum(len(p) for p, _, _ in res[2]) == 8359

    # the raw call: cap = 0 (pix may be NULL) and a cap below need
    n = len(gold[100]["pts"])
    inp = WideInput()
    inp.masks, inp.M, inp.on_device = m5.ctypes.data, 5, 0
    off = np.array([0, n], np.int64)
    for cap in (0, 100):
        pix, dep, pid = np.full(max(cap, 1), -7, np.int64), np.zeros(max(cap, 1)), np.full(max(cap, 1), -7, np.int64)
        car_off, need, ovf = np.zeros(6, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int32)
        o = DepthMapsOutputs()
        o.pix, o.depth, o.point_idx = (pix.ctypes.data, dep.ctypes.data, pid.ctypes.data) if cap else (None, None, None)
        o.cap, o.car_off, o.need, o.overflow, o.on_device = cap, car_off.ctypes.data, need.ctypes.data, ovf.ctypes.data, 0
        ctx._check(ctx._lib.lpf_depth_maps(ctx._h, gold[100]["pts"].ctypes.data, off.ctypes.data, 1, 0, ctypes.byref(inp), ctypes.byref(o)))
        assert need[0] == 8359 and ovf[0] == 1 and car_off[-1] == 8359
        assert np.array_equal(car_off, np.load(os.path.join(GOLDEN, "frame_0000000100.npz"))["depthmap_off_rect5"])
        if cap:
            assert np.array_equal(pix[:cap], np.load(os.path.join(GOLDEN, "frame_0000000100.npz"))["depthmap_idx_rect5"][:cap])
    # the binding retries once with the exact capacity
    full = ctx.depth_maps([gold[100]["pts"]], m5, cap=100)[0]
    assert sum(len(p) for p, _, _ in full) == 8359

    # refusals
    def call(F=1, M=5, cap=10, car=True, need_=True, pix_=True):
        o = DepthMapsOutputs()
        buf = np.zeros(64, np.int64)
        o.pix = buf.ctypes.data if pix_ else None
        o.cap, o.car_off, o.need, o.on_device = cap, buf.ctypes.data if car else None, buf.ctypes.data if need_ else None, 0
        i = WideInput()
        i.masks, i.M, i.on_device = m5.ctypes.data, M, 0
        return ctx._lib.lpf_depth_maps(ctx._h, gold[100]["pts"].ctypes.data, off.ctypes.data, F, 0, ctypes.byref(i), ctypes.byref(o))
    assert call(F=-1) == -1 and call(M=257) == -1 and call(M=-1) == -1 and call(cap=-1) == -1
    assert call(car=False) == -1 and call(need_=False) == -1 and call(pix_=False) == -1
    assert call(pix_=False, cap=0) == 0 and call(F=0) == 0
    with LpfContext(0) as bare:                                 # no camera
        o = DepthMapsOutputs()
        buf = np.zeros(64, np.int64)
        o.car_off, o.need = buf.ctypes.data, buf.ctypes.data
        assert bare._lib.lpf_depth_maps(bare._h, None, off.ctypes.data, 1, 0, ctypes.byref(WideInput()), ctypes.byref(o)) == -3


# ---- 6. state -------------------------------------------------------------------------------------------------------------------
def test_leaves_the_narrow_state_and_refuses_capture(cal, gold):
    fr = gold[100]
    g = load_golden(100)
    with LpfContext(0) as c:
        c.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, 50.0)
        c.set_masks(fr["rect5"])
        c.set_boxes([g["corners_velo"]])
        before = c.run(fr["pts"], want_float=True)
        c.depth_maps([fr["pts"], gold[250]["pts"]], np.stack([_mask_set(gold, 40, 3, cal["W"], cal["H"], False)] * 2), erode_iters=1)
        after = c.run(fr["pts"], want_float=True)
        for k, v in before.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, after[k]), k
        assert all(np.array_equal(a, b) for a, b in zip(before["inst_lists"], after["inst_lists"]))

        good = lambda: c.depth_maps([fr["pts"]], fr["rect5"])[0]   # noqa: E731
        ref = good()
        c.graph_begin()
        o = DepthMapsOutputs()
        buf = np.zeros(64, np.int64)
        o.car_off, o.need = buf.ctypes.data, buf.ctypes.data
        off = np.array([0, len(fr["pts"])], np.int64)
        rc = c._lib.lpf_depth_maps(c._h, fr["pts"].ctypes.data, off.ctypes.data, 1, 0, ctypes.byref(WideInput()), ctypes.byref(o))
        assert rc == -3, rc                                     # LPF_ERR_STATE: the capture is abandoned
        assert "captured" in (c._lib.lpf_last_error(c._h) or b"").decode()
        _same(good(), ref, "after the refused capture")


def test_pipelined_steps_and_depth_maps(cal, gold):
    import torch
    order = [100, ("full", 1461), ("full", 2449)]

    def steps(ctx, keep):
        outs = []
        for k in order:
            fr = gold[k]
            n = len(fr["pts"])
            dp, dm, dr = _dev(fr["pts"]), _dev(fr["rect5"]), _dev(LpfContext.mask_rects(fr["rect5"]))
            no = dict(uv=torch.empty((n, 2), dtype=torch.int32, device="cuda"), label_bits=torch.empty(n, dtype=torch.int32, device="cuda"),
                      valid_idx=torch.empty(n, dtype=torch.int64, device="cuda"), inst_idx=torch.empty((1, n), dtype=torch.int64, device="cuda"),
                      summary=torch.empty(SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda"))
            for t in no.values():                               # what a kernel does not write stays as it is, in both contexts
                t.view(torch.uint8).fill_(0xA5)
            keep.append((dp, dm, dr, no))
            outs.append((ctx.make_frame_step(dp, masks_u8=dm, mask_rects=dr, inst_cap=n, **no), no))
        return outs

    keep = []
    with LpfContext(0) as ref:
        ref.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, DMAX)
        want = []
        for step, no in steps(ref, keep):
            step()
            ref.sync()
            want.append({k: t.cpu().numpy().copy() for k, t in no.items()})
        want_dm = ref.depth_maps([gold[k]["pts"] for k in order], np.stack([gold[k]["rect5"] for k in order]))
    with LpfContext(0) as c:
        c.set_pipelined("fused-pack")
        c.set_camera(cal["T"], cal["K"], cal["W"], cal["H"], 0.0, DMAX)
        jobs = steps(c, keep)
        for step, _ in jobs:                                    # warm-up: every buffer reaches its size
            step()
        c.sync()
        for step, _ in jobs:
            step()
        dm = c.depth_maps([gold[k]["pts"] for k in order], np.stack([gold[k]["rect5"] for k in order]))
        c.sync()
        for (_, no), w in zip(jobs, want):
            for k, t in no.items():
                assert np.array_equal(t.cpu().numpy(), w[k]), k
    for a, b in zip(dm, want_dm):
        _same(a, b, "pipelined")


# ---- 7. reader Scans and GPU masks ------------------------------------------------------------------------------------------------
def test_scans_and_gpu_masks_equal_the_host_path(ctx, cal, gold, tmp_path):
    keys = [100, ("full", 1461), 250]
    paths = []
    for i, k in enumerate(keys):
        p = tmp_path / ("%d.bin" % i)
        gold[k]["pts"].tofile(str(p))
        paths.append(str(p))
    cam = _Cam(cal)
    host = pipeline.depth_maps_frames([pipeline.FrameInputs(i, gold[k]["pts"], list(gold[k]["edge"].astype(np.float32)))
                                       for i, k in enumerate(keys)], cal["T"], cam, DMAX, ctx=ctx)
    with ScanReader(ctx, paths, max_points=200_000) as rd:
        for i, (k, scan) in enumerate(zip(keys, rd)):
            got = pipeline.depth_maps_frames([pipeline.FrameInputs(i, scan, _dev(gold[k]["edge"]))], cal["T"], cam, DMAX, ctx=ctx)[0]
            assert [c for c, _ in got] == [c for c, _ in host[i]]
            _same([(s.pixels, s.depth, s.point_idx) for _, s in got], [(s.pixels, s.depth, s.point_idx) for _, s in host[i]], k)
    # more than 256 masks: groups of 256, concatenated
    m = np.concatenate([gold[100]["rect5"]] * 60)               # 300 masks
    got = pipeline.depth_maps_frames([pipeline.FrameInputs(0, gold[100]["pts"], m)], cal["T"], cam, DMAX, ctx=ctx)[0]
    assert [c for c, _ in got] == list(range(1, 301))
    ref = pipeline.depth_maps_frames([pipeline.FrameInputs(0, gold[100]["pts"], m[:5])], cal["T"], cam, DMAX, ctx=ctx)[0]
    for i, (_, s) in enumerate(got):
        assert np.array_equal(s.pixels, ref[i % 5][1].pixels)


# ---- 8. the frame loop --------------------------------------------------------------------------------------------------------------
def test_process_frames_depth_maps(cal, gold, tmp_path, monkeypatch):
    from test_gpu_pipeline import _dataset_tree
    root, seq, cam, velo, g = _dataset_tree(tmp_path, cal["calib"], (100, 250, 1461, 2717))
    monkeypatch.setattr(pipeline, "sequence_setup", lambda path, s=0, c=0: (seq, cam, cal["calib"]["TrVeloToCam"], cal["T"], velo))

    def segmenter(image_path):
        frame = int(os.path.basename(image_path).split(".")[0])
        m = gold[frame]["rect5"]
        return None, (None if frame == 250 else m.astype(np.float32)), None, None, None
    with contextlib.redirect_stdout(io.StringIO()) as out:
        res = list(pipeline.process_frames_depth_maps(0, 0, segmenter=segmenter, kitti360_path=str(root), frames=[100, 250, 1461, 2717]))
    assert [f for f, _ in res] == [100, 1461]                   # 250: no detections; 2717: its masks are empty
    assert "[INFO] No cars detected in frame 250, skipping." in out.getvalue()
    assert "[INFO] No cars detected in frame 2717, skipping." in out.getvalue()
    for f, cars in res:
        want = pipeline.depth_maps_frames([pipeline.FrameInputs(f, gold[f]["pts"], gold[f]["rect5"].astype(np.float32))], cal["T"], cam, DMAX)[0]
        assert [c for c, _ in cars] == [c for c, _ in want]
        _same([(s.pixels, s.depth, s.point_idx) for _, s in cars], [(s.pixels, s.depth, s.point_idx) for _, s in want], f)
    os.remove(os.path.join(str(root), "data_2d_raw", seq, "image_00", "data_rect", "%010d.png" % 1461))
    with pytest.raises(RuntimeError, match="Image file .*0000001461.png does not exist!"):
        with contextlib.redirect_stdout(io.StringIO()):
            list(pipeline.process_frames_depth_maps(0, 0, segmenter=segmenter, kitti360_path=str(root), frames=[100, 1461]))


# ---- 9. INTEGRATION.md section H runs as written --------------------------------------------------------------------------------
def test_integration_snippet_h():
    text = open(os.path.join(os.path.dirname(GOLDEN), "..", "INTEGRATION.md")).read()
    sec = text[text.index("## H."):]
    code = sec[sec.index("```python") + len("```python"):]
    code = code[:code.index("```")]
    ns = {}
    exec(compile(code, "INTEGRATION.md#H", "exec"), ns)
    assert ns.get("ok") is True
