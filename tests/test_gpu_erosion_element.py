"""lpf_set_erosion_element on the GPU: the k x k MORPH_ELLIPSE erosion of every path that erodes -- the label image of
lpf_set_masks_* (host arrays and device tensors, every binarize rule), the wide and multi-camera passes, lpf_depth_maps,
lpf_erode_masks_u8 and pipeline.run_frames' ``erosion_kernel_size`` -- against tests/erosion_ref.py (the NumPy restatement,
tests/test_erosion_element.py), bit for bit.  Cameras are set to small images so that the 64 x 16 tiles' edges and halos are hit."""
import numpy as np
import pytest

import erosion_ref as R
from conftest import load_golden, unpack_masks
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd._native import LpfContext, LpfError
from oracle import cpu_oracle as orc

pytestmark = pytest.mark.gpu

ODD = np.array([0.0, 0.5, 0.50000006, 0.999, 1.0, 1.5, 2.0, 256.0, np.nan, -1.0], np.float32)
RULE = {"astype": 0, "v3": 1, "gt0.5": 2}
KS = [1, 5, 7, 9, 15]
ITERS = [0, 1, 2, 3]
I_FULL, I_EMPTY, I_RECT, I_DISK, I_RANDOM, I_HALF, I_RECT_RANDOM = range(7)


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


def _camera(ctx, calib, W, H, dmax=50.0):
    """the calibration's camera scaled to a W x H image"""
    K = np.diag([W / float(calib["width"]), H / float(calib["height"]), 1.0]) @ np.asarray(calib["K"], np.float64)[:3, :3]
    ctx.set_camera(calib["TrVeloToRect"], K, W, H, 0.0, dmax)
    return K


def _base_masks(H, W, seed=0):
    """uint8 0 / 1 [7,H,W]: full, empty, a rectangle inset by H/8, W/10, a disk, random < 0.985, the left half with one hole,
    rectangle AND random"""
    rng = np.random.default_rng(1000 * H + W + seed)
    m = np.zeros((7, H, W), np.uint8)
    m[I_FULL] = 1
    m[I_RECT, H // 8:H - H // 8, W // 10:W - W // 10] = 1
    yy, xx = np.mgrid[:H, :W]
    m[I_DISK] = ((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2 <= (0.45 * min(H, W)) ** 2 + 1)
    m[I_RANDOM] = rng.random((H, W)) < 0.985
    m[I_HALF, :, :max(W // 2, 1)] = 1
    m[I_HALF, H // 2, W // 4] = 0
    m[I_RECT_RANDOM] = m[I_RECT] & (rng.random((H, W)) < 0.985)
    return m


def _as_mode(base, mode, seed=3):
    """(the masks as ``mode`` hands them to set_masks, set_masks' binarize, the members the reference's rule makes of them)"""
    if mode == "u8":
        return base * np.uint8(255), None, base
    m = base.astype(np.float32)
    m[I_DISK] *= np.random.default_rng(seed).choice(ODD, size=base.shape[1:])
    return m, mode, orc.binarize_f32(m, RULE[mode])


_REF = {}


def _expected(key, member, k, iters):
    """orc.pack_masks of the eroded members, computed once per (masks, k, iters)"""
    full = (key, k, iters)
    if full not in _REF:
        H, W = member.shape[-2:]
        er = R.erode(member, k, iters)
        _REF[full] = (er, orc.pack_masks(er, 0, H, W))
    return _REF[full]


def _not_vacuous(member, er, H, k, iters):
    if H >= 37 and k <= 9 and iters <= 2:
        assert er[I_FULL].all()
        for i in (I_RECT, I_HALF):
            assert er[i].any(), (i, k, iters)
            if k > 1 and iters > 0:
                assert not np.array_equal(er[i], member[i]), (i, k, iters)


@pytest.mark.parametrize("mode", ["u8", "astype", "v3", "gt0.5"])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (16, 64), (17, 65), (37, 150)], ids=lambda s: "%dx%d" % s)
def test_label_image(ctx, calib, size, mode):
    H, W = size
    _camera(ctx, calib, W, H)
    masks, binarize, member = _as_mode(_base_masks(H, W), mode)
    try:
        for k in KS:
            ctx.set_erosion_element(k)
            for iters in ITERS:
                ctx.set_masks(masks, erode_iters=iters, binarize=binarize)
                er, want = _expected((H, W, mode), member, k, iters)
                _not_vacuous(member, er, H, k, iters)
                assert np.array_equal(ctx.get_label_image()[0], want), (k, iters)
    finally:
        ctx.set_erosion_element(3)


@pytest.mark.parametrize("k,iters,mode", [(5, 1, "u8"), (9, 2, "v3")])
def test_label_image_at_camera_size(ctx, calib, k, iters, mode):
    """376 x 1408: the size at which the 3x3 path takes the streaming pack (hw % 16 == 0); the k x k element packs by tiles"""
    H, W = 376, 1408
    _camera(ctx, calib, W, H)
    masks, binarize, member = _as_mode(_base_masks(H, W), mode)
    er, want = _expected((H, W, mode), member, k, iters)
    _not_vacuous(member, er, H, k, iters)
    try:
        ctx.set_erosion_element(k)
        ctx.set_masks(masks, erode_iters=iters, binarize=binarize)
        assert np.array_equal(ctx.get_label_image()[0], want)
    finally:
        ctx.set_erosion_element(3)


def test_label_image_of_two_frames_and_17_masks(ctx, calib):
    """F = 2, M = 17: 32-bit label words (M <= 8 has bytes, M <= 16 halfwords) and the frame axis of the grid"""
    H, W = 37, 150
    _camera(ctx, calib, W, H)
    a, b = _base_masks(H, W), _base_masks(H, W, seed=5)
    batch = np.stack([np.concatenate([a, b, a[2:5]]), np.concatenate([b, a, b[2:5]])])
    try:
        for M in (9, 17):
            for k, iters in [(5, 1), (7, 2)]:
                ctx.set_erosion_element(k)
                ctx.set_masks(np.ascontiguousarray(batch[:, :M]) * np.uint8(255), erode_iters=iters)
                got = ctx.get_label_image()
                for f in range(2):
                    assert np.array_equal(got[f], orc.pack_masks(R.erode(batch[f, :M], k, iters), 0, H, W)), (M, k, iters, f)
    finally:
        ctx.set_erosion_element(3)


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("size", [(17, 65), (37, 150)], ids=lambda s: "%dx%d" % s)
def test_label_image_from_device_tensors(ctx, calib, size, dtype):
    import torch
    H, W = size
    _camera(ctx, calib, W, H)
    mode = "u8" if dtype == "uint8" else "v3"
    masks, binarize, member = _as_mode(_base_masks(H, W), mode)
    t = torch.from_numpy(masks).cuda()
    torch.cuda.synchronize()
    try:
        for k in (5, 9):
            ctx.set_erosion_element(k)
            for iters in (1, 2):
                for lend in (False, True):
                    ctx.set_masks(t, erode_iters=iters, binarize=binarize, lend=lend)
                    er, want = _expected((H, W, mode), member, k, iters)
                    _not_vacuous(member, er, H, k, iters)
                    assert np.array_equal(ctx.get_label_image()[0], want), (k, iters, lend)
    finally:
        ctx.set_erosion_element(3)


def test_element_state(ctx, calib):
    H, W = 37, 150
    _camera(ctx, calib, W, H)
    base = _base_masks(H, W)
    assert ctx.erosion_kernel_size == 3
    try:
        ctx.set_erosion_element(5)
        ctx.set_masks(base, erode_iters=2)
        five = ctx.get_label_image()[0]
        assert np.array_equal(five, _expected((H, W, "u8"), base, 5, 2)[1])
        for bad in (0, 4, 17, -1, 16):
            with pytest.raises(LpfError, match="ksize=%d" % bad):
                ctx.set_erosion_element(bad)
            assert ctx.erosion_kernel_size == 5
        ctx.set_masks(base, erode_iters=2)                   # a refused size left the element as it was
        assert np.array_equal(ctx.get_label_image()[0], five)
        ctx.set_erosion_element(3)                           # back to the cross: the oracle's own erosion again
        for iters in (0, 1, 2):
            ctx.set_masks(base, erode_iters=iters)
            assert np.array_equal(ctx.get_label_image()[0], orc.pack_masks(base, iters, H, W)), iters
        assert not np.array_equal(orc.pack_masks(base, 2, H, W), five)
        # masks that are packed keep what they were packed with
        ctx.set_erosion_element(7)
        assert np.array_equal(ctx.get_label_image()[0], orc.pack_masks(base, 2, H, W))
    finally:
        ctx.set_erosion_element(3)


def _same(a, b, what=""):
    """two results of the same call, field for field (floats by their bits)"""
    assert type(a) is type(b) or (isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer))), (what, type(a), type(b))
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for key in a:
            _same(a[key], b[key], "%s.%s" % (what, key))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), what
    else:
        assert a == b, (what, a, b)


def _disk_masks(M, H, W, seed):
    """M overlapping disks and boxes, uint8 0 / 1 (big enough to survive a 5 x 5 erosion)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((M, H, W), np.uint8)
    for i in range(M):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.12, 0.35) * H
        m[i] = ((yy - cy) ** 2 + ((xx - cx) / 2.0) ** 2 <= rad * rad) if i % 3 else (abs(yy - cy) <= rad) & (abs(xx - cx) <= 2 * rad)
        m[i] &= rng.random((H, W)) < 0.995
    return m


ALL = dict(want_uv=True, want_float=True, want_lists=True, want_valid_uv=True)


def test_run_wide_equals_host_erosion(calib):
    g = load_golden(100)
    H, W, M = 80, 300, 70
    with LpfContext(0) as c:
        _camera(c, calib, W, H)
        c.set_boxes([np.asarray(g["corners_velo"], np.float64)], oriented=True)
        base = _disk_masks(M, H, W, 4)
        fm = base.astype(np.float32) * np.random.default_rng(2).choice(np.array([0.6, 1.0, 2.5], np.float32), size=(M, 1, 1))
        member = orc.binarize_f32(fm, RULE["v3"])
        er = R.erode(member, 5, 1)
        assert er.any() and not np.array_equal(er, member)
        c.set_erosion_element(5)
        got = c.run_wide([g["points"]], fm, erode_iters=1, binarize="v3", **ALL)
        two = c.run_wide([g["points"]], fm, erode_iters=2, binarize="v3", **ALL)
        want = c.run_wide([g["points"]], er, erode_iters=0, **ALL)
        want2 = c.run_wide([g["points"]], R.erode(member, 5, 2), erode_iters=0, **ALL)
        assert got[0]["n_labelled"] > 0
        _same(got, want, "run_wide")
        _same(two, want2, "run_wide, 2 iterations")
        c.set_erosion_element(3)
        _same(c.run_wide([g["points"]], fm, erode_iters=1, binarize="v3", **ALL),
              c.run_wide([g["points"]], R.erode(member, 3, 1), erode_iters=0, **ALL), "run_wide, back to the cross")


def test_run_cams_equals_host_erosion(calib):
    g = load_golden(100)
    boxes = [np.asarray(g["corners_velo"], np.float64)]
    sizes = [(80, 300), (37, 150)]
    with LpfContext(0) as c:
        specs, eroded = [], []
        for j, (H, W) in enumerate(sizes):
            K = _camera(c, calib, W, H)
            base = _disk_masks(5 + 6 * j, H, W, 10 + j)
            spec = dict(T_velo_to_rect=calib["TrVeloToRect"], K=K, width=W, height=H, depth_min=0.0, depth_max=50.0, boxes=boxes, oriented=True)
            er = R.erode(base, 5, 1)
            assert er.any() and not np.array_equal(er, base)
            specs.append(dict(spec, masks=base * np.uint8(255) if j == 0 else base.astype(np.float32), binarize="astype", erode_iters=1))
            eroded.append(dict(spec, masks=er, erode_iters=0))
        kw = dict(want_uv=True, want_label=True, want_float=True, want_lists=True, want_valid_uv=True)
        c.set_erosion_element(5)
        got = c.run_cams([g["points"]], specs, **kw)
        want = c.run_cams([g["points"]], eroded, **kw)
        assert all(r[0]["n_labelled"] > 0 for r in want)
        _same(got, want, "run_cams")
        wide = c.run_cams_wide([g["points"]], specs, **ALL)
        _same(wide, c.run_cams_wide([g["points"]], eroded, **ALL), "run_cams_wide")


@pytest.mark.parametrize("M", [5, 40])
def test_depth_maps_equals_host_erosion(calib, M):
    g = load_golden(100)
    H, W = 80, 300
    with LpfContext(0) as c:
        _camera(c, calib, W, H)
        base = _disk_masks(M, H, W, 21)
        er = R.erode(base, 5, 1)
        c.set_erosion_element(5)
        got = c.depth_maps([g["points"]], base, binarize="astype", erode_iters=1)
        want = c.depth_maps([g["points"]], er, binarize="astype", erode_iters=0)
        assert any(len(car[0]) for car in want[0])
        _same(got, want, "depth_maps")
        c.set_erosion_element(1)                             # the 1 x 1 element: any number of iterations is the identity
        _same(c.depth_maps([g["points"]], base, binarize="astype", erode_iters=3),
              c.depth_maps([g["points"]], base, binarize="astype", erode_iters=0), "depth_maps, k = 1")


@pytest.mark.parametrize("shape", [(1, 9), (9, 1), (23, 37), (2, 3, 40, 70)], ids=str)
def test_erode_masks_values(ctx, shape):
    import torch
    a = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    a[..., :shape[-2] // 2 + 1, :shape[-1] // 2 + 1] |= 0x80     # (a bright region: the minimum is not 0 everywhere)
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    try:
        for k in (5, 7):
            ctx.set_erosion_element(k)
            for iters in (1, 2):
                want = R.erode(a, k, iters)
                got = ctx.erode_masks(a, iters)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (k, iters)
                assert np.array_equal(ctx.erode_masks(t, iters).cpu().numpy(), want), (k, iters, "device")
        assert R.erode(a, 5, 1).any() or min(shape[-2:]) == 1
        ctx.set_erosion_element(1)
        assert np.array_equal(ctx.erode_masks(a, 4), a)
    finally:
        ctx.set_erosion_element(3)
    assert np.array_equal(ctx.erode_masks(a, 1), R.erode(a, 3, 1))


def _cam(calib):
    return kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))


def _equal_frames(a, b):
    assert a["car_statistics"] == b["car_statistics"]
    assert np.array_equal(a["valid_indices"], b["valid_indices"]) and np.array_equal(a["count_mb"], b["count_mb"])
    assert len(a["car_point_sets"]) == len(b["car_point_sets"])
    assert all(np.array_equal(x, y) for x, y in zip(a["car_point_sets"], b["car_point_sets"]))
    assert np.array_equal(a["bg_assigned"], b["bg_assigned"])


def test_run_frames_with_erosion_kernel_size(calib):
    g = load_golden(100)
    cam = _cam(calib)
    masks = unpack_masks(g, "rect5", cam.height, cam.width)                # float32 [5,H,W], 0 / 1
    boxes = [{"corners_velo": c.tolist()} for c in g["corners_velo"]]
    T = calib["TrVeloToRect"]

    def run(m, **kw):
        return pipeline.run_frames([pipeline.FrameInputs(100, g["points"], m, boxes)], T, cam, 50.0, 10, True, **kw)[0]

    today = run(masks, erode_iters=1, v3_pipeline=True)
    host = R.erode(orc.binarize_f32(masks, RULE["v3"]), 5, 1)
    assert host.any() and not np.array_equal(host, R.erode(orc.binarize_f32(masks, RULE["v3"]), 3, 1))
    got = run(masks, erode_iters=1, v3_pipeline=True, erosion_kernel_size=5)
    _equal_frames(got, run(host))
    assert any(d["total_points"] for d in got["car_statistics"]) and got["car_statistics"] != today["car_statistics"]
    # masks that are not at the camera's size: eroded at their own size (V3:82-97), then resized (V3:222)
    small = np.ascontiguousarray(masks[:, ::2, ::2])
    u8 = (small * 255).astype(np.uint8)
    chain = (R.erode(u8, 5, 1).astype(np.float32) / 255.0).astype(np.uint8)
    _equal_frames(run(small, erode_iters=1, v3_pipeline=True, erosion_kernel_size=5), run(chain))
    # a default call after these: today's result, the element did not leak
    _equal_frames(run(masks, erode_iters=1, v3_pipeline=True), today)
    assert pipeline.get_context(0).erosion_kernel_size == 3
    with pytest.raises(ValueError, match="erosion_kernel_size"):
        run(masks, erode_iters=1, erosion_kernel_size=4)


def test_a_captured_graph_keeps_its_element(calib):
    """The element is a kernel argument: a hipGraph captured with the 5 x 5 element erodes with it on every replay, whatever the
    context's element has become since."""
    import torch
    from lidar_object_detection_amd import synthetic as S
    from lidar_object_detection_amd._native import SUMMARY_DTYPE
    _, T, K, W, H = S.default_calibration(calib)
    n, M, Bx = 150_000, 6, 9
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), LpfContext(0) as c:
        c.set_stream(stream.cuda_stream)
        c.set_camera(T, K, W, H, 0.0, 50.0)
        sc0 = S.scene(n, n_masks=M, n_boxes=Bx, seed=500)
        c.set_boxes(sc0["corners_velo"])
        pts = torch.from_numpy(sc0["points"]).to(dev)
        masks = torch.from_numpy(sc0["masks"]).to(dev)
        o = dict(uv=torch.empty((n, 2), dtype=torch.int32, device=dev), label_bits=torch.empty(n, dtype=torch.int32, device=dev),
                 valid_idx=torch.empty(n, dtype=torch.int64, device=dev), inst_idx=torch.empty(n, dtype=torch.int64, device=dev),
                 count_mb=torch.zeros(M * Bx, dtype=torch.int32, device=dev),
                 summary=torch.zeros(SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev))
        c.set_erosion_element(5)
        step = c.make_device_step(pts, np.array([0, n], np.int64), masks_u8=masks.unsqueeze(0), erode_iters=2, inst_cap=n, **o)
        step()                                               # warm: allocations + table uploads happen here
        c.sync()
        c.graph_begin()
        step()
        g = c.graph_end()
        c.set_erosion_element(3)
        sc = S.scene(n, n_masks=M, n_boxes=Bx, seed=501)
        pts.copy_(torch.from_numpy(sc["points"]))
        masks.copy_(torch.from_numpy(sc["masks"]))
        stream.synchronize()
        c.graph_launch(g)
        c.sync()
        member = (sc["masks"] != 0).astype(np.uint8)
        five = orc.pack_masks(R.erode(member, 5, 2), 0, H, W)
        assert not np.array_equal(five, orc.pack_masks(member, 2, H, W))
        ref = orc.run(sc["points"], T, K, W, H, 0.0, 50.0, label_img=five, M=M, corners=sc0["corners_velo"], want_float=False)
        assert np.count_nonzero(ref["label_bits"]) > 0
        assert np.array_equal(o["label_bits"].cpu().numpy().view(np.uint32), ref["label_bits"])
        assert np.array_equal(o["count_mb"].cpu().numpy().reshape(M, Bx), ref["count_mb"])
        step()                                               # outside the graph the step now erodes with the cross again
        c.sync()
        ref3 = orc.run(sc["points"], T, K, W, H, 0.0, 50.0, label_img=orc.pack_masks(member, 2, H, W), M=M, corners=sc0["corners_velo"], want_float=False)
        assert np.array_equal(o["label_bits"].cpu().numpy().view(np.uint32), ref3["label_bits"])
        c.graph_destroy(g)
