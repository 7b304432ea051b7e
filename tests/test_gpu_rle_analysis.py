"""Run-length masks through the two analysis calls on the GPU (lpf_depth_maps_rle, lpf_first_match_rle; LpfContext.depth_maps /
first_match and pipeline.depth_maps_frames / first_match_frames on top).  The yardstick of every case but the last is the existing
dense call on the ``to_dense()`` uint8 host masks in the same process: every output array equal, the unwritten entries too (both sides
start from the same fill).  Independently the first-mask codes and the depth maps' pixel sets, winners and depths are recomputed in
NumPy from the projected ``uv`` (lpf_run_wide without masks) and the runs' membership (tests/rle_ref.py).  The clouds are a
back-projection of EVERY pixel centre plus noise points, twice over at different depths, and the tests assert from ``uv`` that every
pixel of every frame receives a valid point.  Images: 37 x 23 (851 pixels: no multiple of 64 or 1024) and 160 x 48.  The last case
-- 16 frames of 256 one-run masks at 1408 x 376, 271 MB of label planes against the 256 MiB of a range -- has a closed-form yardstick."""
import numpy as np
import pytest

import rle_ref as R
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd._native import LpfContext, LpfError
from lidar_object_detection_amd.rle import RleMasks
from test_gpu_wide_rle import LARGE, MID, SMALL, T, _cloud, _K, _masks, _rles, _same, _scrambled

pytestmark = pytest.mark.gpu

MS = [0, 1, 31, 32, 33, 64, 65, 255, 256]
NARROW = dict(want_uv=True, want_label=True, want_float=True, want_lists=True, want_valid_uv=True)
FM_WANT = ("first_mask", "car_idx", "car_mask", "car_xyz", "car_rgb", "bg_idx", "bg_xyz", "n_valid", "n_car", "n_bg", "mask_count")


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


def _setup(c, W, H):
    c.set_erosion_element(3)
    c.set_camera(T, _K(W, H), W, H, 0.0, 50.0)
    c.clear_boxes()


_two = {}


def _cloud2(W, H, F):
    """_cloud's frames, two of them per frame: every pixel gets two grid points at different depths (the last writer matters)"""
    if (W, H, F) not in _two:
        a = _cloud(W, H, F + 1)
        _two[(W, H, F)] = [np.ascontiguousarray(np.concatenate([a[f], a[f + 1]])) for f in range(F)]
    return _two[(W, H, F)]


_proj_cache = {}


def _proj(c, pts, W, H, key=None):
    """per frame (u, v, depth, valid_idx) of the points, from lpf_run_wide without masks (the camera is set)"""
    if key is None or key not in _proj_cache:
        res = c.run_wide(pts, np.zeros((len(pts), 0, H, W), np.uint8), want_uv=True, want_float=True, want_lists=True, want_valid_uv=True)
        out = [(r["u"].astype(np.int64), r["v"].astype(np.int64), r["depth"], r["valid_idx"]) for r in res]
        if key is None:
            return out
        _proj_cache[key] = out
    return _proj_cache[key]


def _every_pixel_is_hit(proj, W, H):
    for u, v, _, vi in proj:
        hit = np.zeros((H, W), bool)
        hit[v[vi], u[vi]] = True
        assert hit.all()


_mem_cache = {}


def _members(rles, key=None):
    """bool [M,h,w] per frame from the runs, by tests/rle_ref.py's loops (computed once per key)"""
    if key is None or key not in _mem_cache:
        out = [R.masks_to_dense(r.runs, r.run_off, *r.shape).astype(bool) for r in rles]
        if key is None:
            return out
        _mem_cache[key] = out
    return _mem_cache[key]


def _codes(members, u, v, vi, n):
    """first-mask codes of one frame: -2 not valid, -1 background, else the first mask whose plane [mh, mw] holds the pixel"""
    M, mh, mw = members.shape
    code = np.full(n, -2, np.int32)
    c = np.full(len(vi), -1, np.int32)
    inside = (u[vi] < mw) & (v[vi] < mh)
    if M and inside.any():
        mem = members[:, v[vi][inside], u[vi][inside]]
        c[inside] = np.where(mem.any(axis=0), mem.argmax(axis=0), -1)
    code[vi] = c
    return code


def _fm_is_right(res, pts, proj, members, colors=None):
    """a first_match result against the codes recomputed from uv and the members"""
    off = res["frame_off"]
    for f, (u, v, _, vi) in enumerate(proj):
        a, n = int(off[f]), len(pts[f])
        code = _codes(members[f], u, v, vi, n)
        assert np.array_equal(res["first_mask"][a:a + n], code), f
        car, bg = np.flatnonzero(code >= 0), np.flatnonzero(code == -1)
        assert res["n_car"][f] == len(car) and res["n_bg"][f] == len(bg) and res["n_valid"][f] == len(vi)
        assert np.array_equal(res["car_idx"][a:a + len(car)], car) and np.array_equal(res["bg_idx"][a:a + len(bg)], bg)
        assert np.array_equal(res["car_mask"][a:a + len(car)], code[car])
        assert np.array_equal(res["car_xyz"][a:a + len(car)], pts[f][car, :3]) and np.array_equal(res["bg_xyz"][a:a + len(bg)], pts[f][bg, :3])
        M = members[f].shape[0]
        assert np.array_equal(res["mask_count"][f], np.bincount(code[car], minlength=M)[:M])
        if colors is not None:
            assert np.array_equal(res["car_rgb"][a:a + len(car)], colors[f][code[car]])


def _colors(F, M):
    return (np.random.default_rng(F * 1000 + M).integers(0, 256, (F, M, 3)).astype(np.uint8) / 255.0).astype(np.float64)


def _dm_is_right(res, proj, members):
    """a depth_maps result (per frame M tuples) against the pixel sets, winners and depths recomputed from uv and the members"""
    for f, (u, v, depth, vi) in enumerate(proj):
        M, H, W = members[f].shape
        win = np.full(H * W, -1, np.int64)
        np.maximum.at(win, v[vi] * W + u[vi], vi)
        assert len(res[f]) == M
        for m, (pix, dep, pid) in enumerate(res[f]):
            want = np.flatnonzero(members[f][m].reshape(-1) & (win >= 0))
            assert np.array_equal(pix, want), (f, m)
            assert np.array_equal(pid, win[want]) and np.array_equal(dep, depth[win[want]]), (f, m)


# ---- depth maps ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", MS)
def test_depth_maps_equals_the_dense_call(ctx, M, F):
    for W, H in (SMALL, MID):
        _setup(ctx, W, H)
        pts = _cloud2(W, H, F)
        dense = _masks(F, M, W, H)
        rles = _rles(dense)
        want = ctx.depth_maps(pts, np.ascontiguousarray(dense), binarize="astype")
        got = ctx.depth_maps(pts, rles)
        _same(got, want)
        proj = _proj(ctx, pts, W, H, (W, H, F))
        _every_pixel_is_hit(proj, W, H)
        _dm_is_right(got, proj, _members(rles, (W, H, F, M)))
        if M:
            assert all(len(cars) == M for cars in got) and sum(len(p) for p, _, _ in got[0]) > 0
            if F == 1:
                _same(ctx.depth_maps(pts, rles[0]), want)        # one RleMasks, not a list


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("iters", [1, 2])
def test_depth_maps_erosion_runs_on_the_decoded_planes(ctx, iters, k):
    for W, H in (SMALL, MID):
        _setup(ctx, W, H)
        ctx.set_erosion_element(k)
        try:
            pts = _cloud2(W, H, 3)
            dense = _masks(3, 65, W, H)
            want = ctx.depth_maps(pts, np.ascontiguousarray(dense), binarize="astype", erode_iters=iters)
            got = ctx.depth_maps(pts, _rles(dense), erode_iters=iters)
            _same(got, want)
            plain = ctx.depth_maps(pts, _rles(dense))
            assert sum(len(p) for cars in got for p, _, _ in cars) < sum(len(p) for cars in plain for p, _, _ in cars)
            assert sum(len(p) for cars in got for p, _, _ in cars) > 0
        finally:
            ctx.set_erosion_element(3)


def _dm_out(F, M, cap, fill=-7):
    import torch
    dev = torch.device("cuda", 0)
    return {"pix": torch.full((F, cap), fill, dtype=torch.int64, device=dev), "depth": torch.full((F, cap), float(fill), dtype=torch.float64, device=dev),
            "point_idx": torch.full((F, cap), fill, dtype=torch.int64, device=dev), "car_off": torch.full((F, M + 1), fill, dtype=torch.int64, device=dev),
            "need": torch.full((F,), fill, dtype=torch.int64, device=dev), "overflow": torch.full((F,), fill, dtype=torch.int32, device=dev)}


@pytest.mark.parametrize("cap", ["fits", "too small"])
def test_depth_maps_device_outputs_and_overflow(ctx, cap):
    import torch
    W, H = MID
    F, M = 3, 65
    _setup(ctx, W, H)
    pts = _cloud2(W, H, F)
    dense = _masks(F, M, W, H)
    rles = _rles(dense)
    need = np.array([int(d.sum()) for d in dense])           # every pixel has a winner: a car's list is its members
    cap = int(need.max()) + 3 if cap == "fits" else int(need.min()) // 2
    want, got = _dm_out(F, M, cap), _dm_out(F, M, cap)
    ctx.depth_maps(pts, np.ascontiguousarray(dense), binarize="astype", cap=cap, out=want)
    ctx.depth_maps(pts, rles, cap=cap, out=got)
    torch.cuda.synchronize()
    for key in want:                                         # the sentinel beyond need / cap too: nothing else was written
        assert np.array_equal(got[key].cpu().numpy(), want[key].cpu().numpy()), key
    assert np.array_equal(got["need"].cpu().numpy(), need)
    assert np.array_equal(got["overflow"].cpu().numpy(), (need > cap).astype(np.int32))
    assert (got["overflow"].cpu().numpy() == 1).all() if cap < need.min() else not got["overflow"].any()
    pix = got["pix"].cpu().numpy()
    for f in range(F):
        assert (pix[f, min(cap, need[f]):] == -7).all() and (pix[f, :min(cap, need[f])] >= 0).all()


def test_depth_maps_shuffled_overlapping_and_repeated_runs(ctx):
    W, H = MID
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 2)
    dense = _masks(2, 65, W, H)
    messy = [_scrambled(r, 5 + i) for i, r in enumerate(_rles(dense))]
    assert all(len(m.runs) > len(r.runs) for m, r in zip(messy, _rles(dense)))
    for iters in (0, 1):
        want = ctx.depth_maps(pts, np.ascontiguousarray(dense), binarize="astype", erode_iters=iters)
        _same(ctx.depth_maps(pts, messy, erode_iters=iters), want)
    _dm_is_right(ctx.depth_maps(pts, messy), _proj(ctx, pts, W, H, (W, H, 2)), _members(messy))


# ---- first match ---------------------------------------------------------------------------------------------------------------

def _fm_both(c, pts, dense, colors=None, want=FM_WANT):
    if colors is None:
        want = tuple(w for w in want if w != "car_rgb")
    a = c.first_match(pts, np.ascontiguousarray(dense), colors, want=want)
    b = c.first_match(pts, _rles(dense), colors, want=want)
    _same(b, a)
    return b


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", MS)
def test_first_match_equals_the_dense_call(ctx, M, F):
    for W, H in (SMALL, MID):
        _setup(ctx, W, H)
        pts = _cloud2(W, H, F)
        dense = _masks(F, M, W, H)
        colors = _colors(F, M)
        got = _fm_both(ctx, pts, dense, colors)
        proj = _proj(ctx, pts, W, H, (W, H, F))
        _every_pixel_is_hit(proj, W, H)
        _fm_is_right(got, pts, proj, _members(_rles(dense), (W, H, F, M)), colors)
        if M:
            assert got["n_car"].min() > 0 and got["n_bg"].min() >= 0
            if F == 1:
                _same(ctx.first_match(pts, _rles(dense)[0], colors[0], want=FM_WANT), got)


def _pixel_points(pix, W, H, depth=7.0):
    """float32 [n,4] points whose projections are the centres of the flat pixels ``pix``"""
    K = _K(W, H)
    xs, ys = (pix % W).astype(np.float64), (pix // W).astype(np.float64)
    z = depth + (pix % 5)
    return np.stack([z, -(xs - K[0, 2]) / K[0, 0] * z, -(ys - K[1, 2]) / K[1, 1] * z, np.zeros(len(pix))], axis=1).astype(np.float32)


def test_first_match_frame_sizes_and_tile_boundaries(ctx):
    """frames of 0, 1, 64, 1023, 1024 and 4097 points; point i sits on pixel 7 i mod hw, and the even ones belong to mask (i / 2) mod M:
    car and background alternate across 63|64, 255|256 and 1023|1024"""
    W, H = MID
    hw, M = W * H, 33
    _setup(ctx, W, H)
    sizes = [0, 1, 64, 1023, 1024, 4097]
    pts, dense = [], np.zeros((len(sizes), M, H, W), np.uint8)
    for f, n in enumerate(sizes):
        i = np.arange(n)
        pix = (i * 7 + f) % hw
        pts.append(_pixel_points(pix, W, H))
        dense[f].reshape(M, -1)[(i[::2] // 2) % M, pix[::2]] = 1
    got = _fm_both(ctx, pts, dense, _colors(len(sizes), M))
    none = np.zeros(0, np.int64)
    proj = [(none, none, np.zeros(0), none)] + _proj(ctx, pts[1:], W, H)          # (frame 0 has no point)
    _fm_is_right(got, pts, proj, _members(_rles(dense)), _colors(len(sizes), M))
    code = got["first_mask"][int(got["frame_off"][5]):]
    for b in (63, 255, 1023):
        assert code[b] == -1 and code[b + 1] == ((b + 1) // 2) % M and code[b - 1] >= 0
    assert list(got["n_car"]) == [0, 1, 32, 512, 512, 2049] and list(got["n_bg"]) == [0, 0, 32, 511, 512, 2048]


def test_first_match_masks_in_different_words(ctx):
    """points held by masks 31 and 32, by masks 0 and 255, and by mask 255 alone; a full-plane single run as mask 32"""
    W, H = SMALL
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 2)
    dense = np.zeros((2, 256, H, W), np.uint8)
    dense[:, 0, :8, :10] = dense[:, 255, :12, :10] = 1       # rows 0..7: 0 and 255; rows 8..11: 255 alone
    dense[:, 31, 14:20, 20:] = dense[:, 32, 14:20, 18:] = 1  # 31 and 32; columns 18, 19: 32 alone
    got = _fm_both(ctx, pts, dense)
    proj = _proj(ctx, pts, W, H, (W, H, 2))
    _fm_is_right(got, pts, proj, _members(_rles(dense)))
    assert set(np.unique(got["first_mask"])) == {-2, -1, 0, 31, 32, 255}
    assert got["mask_count"][0, 255] > 0 and got["mask_count"][0, 32] > 0
    off = np.zeros(34, np.int64)
    off[33] = 1
    full = RleMasks(np.array([[0, W * H]], np.int32), off, (33, H, W))
    one = ctx.first_match(pts[:1], full, want=FM_WANT[:4] + FM_WANT[5:])
    _same(one, ctx.first_match(pts[:1], full.to_dense(), want=FM_WANT[:4] + FM_WANT[5:]))
    valid = one["first_mask"] != -2
    assert valid.any() and (one["first_mask"][valid] == 32).all() and one["n_bg"][0] == 0


def test_first_match_256_masks_on_the_same_pixels_five_times(ctx):
    W, H = SMALL
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 3)
    one = _masks(3, 1, W, H)
    one[:, 0].reshape(3, -1)[:, 100:400] = 1
    dense = np.repeat(one, 256, axis=1)
    want = ctx.first_match(pts, dense, want=FM_WANT[:4] + FM_WANT[5:])
    rles = _rles(dense)
    for _ in range(5):
        _same(ctx.first_match(pts, rles, want=FM_WANT[:4] + FM_WANT[5:]), want)
    assert set(np.unique(want["first_mask"])) == {-2, -1, 0} and (want["mask_count"][:, 1:] == 0).all()


@pytest.mark.parametrize("mh,mw", [(30, 100), (60, 200), (48, 159), (47, 160)])
def test_first_match_masks_smaller_and_larger_than_the_image(ctx, mh, mw):
    W, H = MID
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 2)
    M = 40
    dense = (np.random.default_rng(mh * mw).random((2, M, mh, mw)) < 0.05).astype(np.uint8)
    dense[:, 3, mh - 1, :] = dense[:, 5, :, mw - 1] = 1      # the masks' last row and last column
    got = _fm_both(ctx, pts, dense, _colors(2, M))
    proj = _proj(ctx, pts, W, H, (W, H, 2))
    _every_pixel_is_hit(proj, W, H)                          # so there are valid points at u = mw - 1, mw and v = mh - 1, mh (in the image)
    _fm_is_right(got, pts, proj, _members(_rles(dense)), _colors(2, M))
    u, v, _, vi = proj[0]
    code = got["first_mask"][:len(pts[0])]
    assert (code[vi][(u[vi] == mw - 1) & (v[vi] < mh)] >= 0).all() and (code[vi][(v[vi] == mh - 1) & (u[vi] < mw)] >= 0).all()
    if mw < W:
        assert (code[vi][u[vi] >= mw] == -1).all() and (u[vi] == mw).any()
    if mh < H:
        assert (code[vi][v[vi] >= mh] == -1).all() and (v[vi] == mh).any()


def test_first_match_host_and_device_outputs_keep_what_is_not_written(ctx):
    import torch
    W, H = MID
    F, M = 3, 65
    _setup(ctx, W, H)
    pts = _cloud2(W, H, F)
    dense = _masks(F, M, W, H)
    colors = _colors(F, M)
    n = sum(len(p) for p in pts)
    table = {"first_mask": ("int32", (n,)), "car_idx": ("int64", (n,)), "car_mask": ("int32", (n,)), "car_xyz": ("float32", (n, 3)),
             "car_rgb": ("float64", (n, 3)), "bg_idx": ("int64", (n,)), "bg_xyz": ("float32", (n, 3)), "n_valid": ("int64", (F,)),
             "n_car": ("int64", (F,)), "n_bg": ("int64", (F,)), "mask_count": ("int64", (F, M))}
    host = lambda: {k: np.full(s, -7, dt) for k, (dt, s) in table.items()}
    dev = lambda: {k: torch.full(s, -7, dtype=getattr(torch, dt), device="cuda:0") for k, (dt, s) in table.items()}
    want = ctx.first_match(pts, np.ascontiguousarray(dense), colors, want=FM_WANT, out=host())
    got_h = ctx.first_match(pts, _rles(dense), colors, want=FM_WANT, out=host())
    _same(got_h, want)
    got_d = ctx.first_match(pts, _rles(dense), colors, want=FM_WANT, out=dev())
    got_c = ctx.first_match(pts, _rles(dense), torch.from_numpy(colors).to("cuda:0"), want=FM_WANT)      # GPU colours: GPU outputs of its own
    torch.cuda.synchronize()
    for key in FM_WANT:
        assert np.array_equal(got_d[key].cpu().numpy(), want[key]), key
    nc = int(want["n_car"][0])
    assert (want["car_idx"][nc:len(pts[0])] == -7).all() and (want["car_idx"][:nc] >= 0).all()      # beyond the count: as it was
    for key in ("first_mask", "n_car", "n_bg", "mask_count"):
        assert np.array_equal(got_c[key].cpu().numpy(), want[key]), key
    assert np.array_equal(got_c["car_rgb"].cpu().numpy()[:nc], want["car_rgb"][:nc])


# ---- state, capture, pipeline --------------------------------------------------------------------------------------------------

def _analysis_calls(c, pts, masks, **kw):
    return (c.depth_maps(pts, masks, erode_iters=1, **kw), c.first_match(pts, masks, want=("first_mask", "car_idx", "bg_idx", "mask_count")))


def test_between_two_narrow_runs_the_narrow_state_is_left_alone(ctx):
    W, H = MID
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 2)
    narrow, dense = _masks(2, 5, W, H), _masks(2, 40, W, H)
    ctx.set_masks_rle(_rles(narrow))
    img0 = ctx.get_label_image()
    run0 = ctx.run_batch(pts, **NARROW)
    got = _analysis_calls(ctx, pts, _rles(dense))
    assert np.array_equal(ctx.get_label_image(), img0) and img0.any() and (ctx.M, ctx.F_masks) == (5, 2)
    _same(ctx.run_batch(pts, **NARROW), run0)
    _same(got, _analysis_calls(ctx, pts, np.ascontiguousarray(dense), binarize="astype"))
    ctx.clear_masks()


@pytest.mark.parametrize("mode", ["fused", "fused-pack"])
def test_pipelined_context_with_a_narrow_run_owed(mode):
    """a narrow device run is queued (its tail and summaries ride in later launches), then the two run-length calls: they launch what
    is owed and run in order; then the same again.  All give what a serial context gives"""
    import torch
    W, H = MID
    pts = _cloud2(W, H, 1)
    narrow, dense = _masks(1, 5, W, H), _masks(1, 40, W, H)
    dev = torch.device("cuda", 0)
    n = len(pts[0])
    with LpfContext(0) as serial:
        _setup(serial, W, H)
        serial.set_masks_rle(_rles(narrow))
        want_narrow = serial.run_batch(pts, **NARROW)
        want = _analysis_calls(serial, pts, np.ascontiguousarray(dense), binarize="astype")
        img = serial.get_label_image()
    with LpfContext(0) as c:
        c.set_pipelined(mode)
        _setup(c, W, H)
        tp = torch.from_numpy(pts[0]).to(dev)
        outs = [(torch.zeros((n, 2), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)) for _ in range(2)]
        torch.cuda.synchronize()
        got = []
        for uv, bits in outs:
            c.set_masks_rle(_rles(narrow))
            c.run_device(tp, [0, n], uv=uv, label_bits=bits)
            got.append(_analysis_calls(c, pts, _rles(dense)))
        assert np.array_equal(c.get_label_image(), img) and img.any() and (c.M, c.F_masks) == (5, 1)     # the narrow label image, behind both calls
        c.sync()
        for (uv, bits), g in zip(outs, got):
            _same(g, want)
            assert np.array_equal(uv.cpu().numpy(), np.stack([want_narrow[0]["u"], want_narrow[0]["v"]], axis=1))
            assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_narrow[0]["label_bits"])
        c.set_pipelined(False)


def test_both_calls_are_refused_inside_a_capture(ctx):
    W, H = SMALL
    _setup(ctx, W, H)
    pts = _cloud2(W, H, 1)
    rles = _rles(_masks(1, 5, W, H))
    ctx.depth_maps(pts, rles)
    ctx.first_match(pts, rles)
    ctx.graph_begin()                                        # (a refusal abandons the capture: one capture per call)
    with pytest.raises(LpfError, match="lpf_depth_maps_rle cannot be captured"):
        ctx.depth_maps(pts, rles)
    ctx.graph_begin()
    with pytest.raises(LpfError, match="lpf_first_match_rle cannot be captured"):
        ctx.first_match(pts, rles)
    _same(ctx.depth_maps(pts, rles), ctx.depth_maps(pts, rles[0].to_dense(), binarize="astype"))
    _same(ctx.first_match(pts, rles), ctx.first_match(pts, rles[0].to_dense()))


def _camera(W, H):
    return kitti360.CameraPerspective.from_arrays(_K(W, H), np.eye(3), W, H)


@pytest.mark.parametrize("M", [5, 40, 300])
def test_pipeline_routes_take_the_runs_as_they_are(monkeypatch, M):
    W, H = SMALL
    pts = _cloud2(W, H, 2)
    cam = _camera(W, H)
    both = np.concatenate([_masks(2, 256, W, H), _masks(3, 256, W, H)[1:]], axis=1)      # [2, 512, H, W]
    dense = [both[0, :M], both[1, :max(M - 3, 0)]]           # ragged
    colors = [[(i % 256, (3 * i) % 256, 255 - i % 256) for i in range(len(d))] for d in dense]
    rles = _rles(dense)
    with LpfContext(0) as c:
        frames = lambda masks: [pipeline.FrameInputs(100 + i, p, m, colors=col) for i, (p, m, col) in enumerate(zip(pts, masks, colors))]
        want_dm = pipeline.depth_maps_frames(frames(dense), T, cam, 50.0, ctx=c)
        want_fm = pipeline.first_match_frames(frames(dense), T, cam, 50.0, ctx=c)
        with monkeypatch.context() as mp:
            def no_dense(self_):
                raise AssertionError("RleMasks.to_dense was called: the runs must reach the GPU as runs")
            mp.setattr(RleMasks, "to_dense", no_dense)
            got_dm = pipeline.depth_maps_frames(frames(rles), T, cam, 50.0, ctx=c)
            got_fm = pipeline.first_match_frames(frames(rles), T, cam, 50.0, ctx=c)
    assert [len(fr) for fr in got_dm] == [len(d) for d in dense]
    for fa, fb in zip(got_dm, want_dm):
        for (ia, a), (ib, b) in zip(fa, fb):
            assert ia == ib and a.shape == b.shape
            _same((a.pixels, a.depth, a.point_idx), (b.pixels, b.depth, b.point_idx))
    _same(got_fm, want_fm)
    assert sum(len(a) for _, a in got_dm[0]) > 0 and len(got_fm[0]["car_idx"]) > 0


# ---- the range boundary, with a closed-form yardstick ---------------------------------------------------------------------------

def test_sixteen_large_frames_go_through_in_more_than_one_range(ctx):
    """F = 16 frames at 1408 x 376 with M = 256 one-run masks and 384 points each: 16.9 MB of label planes per frame, so the 256 MiB of
    a range cut the batch (its dense twin would be 2 GB and is not built).  Mask m of frame f is the run [s, s + 40 + f) with
    s = (1009 m + 7919 f) * 31 mod (hw - 128): every frame's runs differ, so a range that decoded another range's runs would be seen.
    Point i of a frame sits on pixel s(m = 2 i mod 256) + (i mod 70): in its run for i mod 70 < 40 + f, else most likely in none."""
    W, H = LARGE
    hw, F, M, N = W * H, 16, 256, 384
    _setup(ctx, W, H)
    start = lambda f: ((1009 * np.arange(M) + 7919 * f) * 31) % (hw - 128)
    rles, pts, members_of = [], [], []
    for f in range(F):
        s, n = start(f), 40 + f
        rles.append(RleMasks(np.stack([s, np.full(M, n)], axis=1).astype(np.int32), np.arange(M + 1, dtype=np.int64), (M, H, W)))
        i = np.arange(N)
        pts.append(_pixel_points(s[(2 * i) % M] + (i % 70), W, H))
        members_of.append((s, n))
    proj = _proj(ctx, pts, W, H)
    fm = ctx.first_match(pts, rles, want=("first_mask", "car_idx", "car_mask", "bg_idx", "n_car", "n_bg", "mask_count"))
    dm = ctx.depth_maps(pts, rles)
    total_car = 0
    for f, (u, v, depth, vi) in enumerate(proj):
        s, n = members_of[f]
        assert len(vi) == N                                  # every point is valid
        pix = v * W + u
        mem = (pix[None, :] >= s[:, None]) & (pix[None, :] < s[:, None] + n)          # [M, N]
        code = np.where(mem.any(axis=0), mem.argmax(axis=0), -1).astype(np.int32)
        a = f * N
        assert np.array_equal(fm["first_mask"][a:a + N], code), f
        car, bg = np.flatnonzero(code >= 0), np.flatnonzero(code == -1)
        assert fm["n_car"][f] == len(car) and fm["n_bg"][f] == len(bg) and len(car) > 200 and len(bg) > 0
        assert np.array_equal(fm["car_idx"][a:a + len(car)], car) and np.array_equal(fm["car_mask"][a:a + len(car)], code[car])
        assert np.array_equal(fm["bg_idx"][a:a + len(bg)], bg)
        assert np.array_equal(fm["mask_count"][f], np.bincount(code[car], minlength=M))
        total_car += len(car)
        win = np.full(hw, -1, np.int64)
        np.maximum.at(win, pix, np.arange(N))
        hit = np.flatnonzero(win >= 0)
        for m in range(M):
            want = hit[(hit >= s[m]) & (hit < s[m] + n)]
            p, d, w = dm[f][m]
            assert np.array_equal(p, want) and np.array_equal(w, win[want]) and np.array_equal(d, depth[win[want]]), (f, m)
    assert total_car > 16 * 200
