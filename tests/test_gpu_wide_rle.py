"""Run-length masks through the wide and multi-camera passes on the GPU (lpf_wide_input.f32 = LPF_MASKS_RLE: lpf_run_wide,
lpf_run_cams_wide, lpf_run_cams; pipeline.run_frames / run_frames_multicam on top).  The yardstick is the same call with the
``to_dense()`` host uint8 masks: every returned array equal.  Alongside it the label words are recomputed in NumPy from the dense masks
(eroded with the cross where the case erodes) at each valid point's pixel.  The clouds are a back-projection of EVERY pixel centre at
mixed depths plus noise points, and the tests assert from ``uv`` that every pixel of every frame receives a valid point: the outputs
expose every element of the label planes.  Images: 37 x 23 (851 pixels: no multiple of 64 or 1024) and 160 x 48."""
import itertools

import numpy as np
import pytest

from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd._native import LpfContext
from lidar_object_detection_amd.rle import RleMasks

pytestmark = pytest.mark.gpu

SMALL, MID, LARGE = (37, 23), (160, 48), (1408, 376)
T = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float64)      # velodyne x forward -> camera z
WANT = dict(want_uv=True, want_float=True, want_lists=True, want_valid_uv=True)
NARROW = dict(want_uv=True, want_label=True, want_float=True, want_lists=True, want_valid_uv=True)


def _K(W, H, f=None):
    f = float(f or W)
    return np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], np.float64)


_clouds = {}


def _cloud(W, H, F, stride=1, K=None):
    """F frames of float32 [N,4] points: one per pixel (x, y) with x, y multiples of ``stride``, back-projected from the pixel's
    centre at a depth of 3 .. 39 m that changes from pixel to pixel, plus hw / 3 noise points (some in view, many not), shuffled"""
    key = (W, H, F, stride, None if K is None else K.tobytes())
    if key not in _clouds:
        K_ = _K(W, H) if K is None else K
        rng = np.random.default_rng(W * 7 + H * 3 + F)
        ys, xs = np.mgrid[0:H:stride, 0:W:stride]
        xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
        frames = []
        for f in range(F):
            z = 3.0 + ((xs * 7 + ys * 13 + f * 5) % 37)
            cx, cy = (xs - K_[0, 2]) / K_[0, 0] * z, (ys - K_[1, 2]) / K_[1, 1] * z
            grid = np.stack([z, -cx, -cy, rng.random(len(z))], axis=1)
            noise = np.concatenate([rng.uniform(-60, 60, (len(z) // 3 + 5, 3)), rng.random((len(z) // 3 + 5, 1))], axis=1)
            pts = np.concatenate([grid, noise]).astype(np.float32)
            frames.append(np.ascontiguousarray(pts[rng.permutation(len(pts))]))
        _clouds[key] = frames
    return _clouds[key]


def _boxes(F):
    """two axis-aligned boxes per frame (velodyne corners [2,8,3]), a little different in every frame"""
    out = []
    for f in range(F):
        b = []
        for lo, hi in (((4, -2, -1.5), (20 + f, 2, 1.5)), ((20, -8 - f, -3), (45, 0, 3))):
            b.append([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i, j, k in itertools.product((0, 1), repeat=3)])
        out.append(np.asarray(b, np.float64))
    return out


_base = {}


def _masks(F, M, W, H):
    """uint8 0 / 1 [F,M,H,W], the same for every caller: rectangles, flat intervals that cross row ends, sparse noise, every fourth mask
    empty, overlaps; the first and the last pixel of every image -- so also of the batch -- belong to the first and the last mask"""
    if (W, H) not in _base:
        rng = np.random.default_rng(W * 1000 + H)
        yy, xx = np.mgrid[:H, :W]
        b = np.zeros((3, 256, H, W), np.uint8)
        for f in range(3):
            for m in range(256):
                kind = (m + f) % 4
                if kind == 0:
                    cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.15, 0.5) * H
                    b[f, m] = (abs(yy - cy) <= r) & (abs(xx - cx) <= 2 * r)
                elif kind == 1:
                    s = int(rng.integers(0, H * W - 1))
                    n = int(rng.integers(1, min(4 * W, H * W - s) + 1))
                    b[f, m].reshape(-1)[s:s + n] = 1                 # a run across row ends
                elif kind == 2:
                    b[f, m] = rng.random((H, W)) < 0.2
                # kind 3: an empty mask
        _base[(W, H)] = b
    d = _base[(W, H)][:F, :M].copy()
    if M:
        d[:, 0, 0, 0] = d[:, 0, H - 1, W - 1] = 1
        d[:, M - 1, 0, 0] = d[:, M - 1, H - 1, W - 1] = 1
    return d


def _rles(dense):
    return [RleMasks.from_dense(d) for d in dense]


def _erode_cross(dense, iters):
    """cv2.erode with the 3 x 3 cross, border pixels' missing neighbours not eroding (cv2's default border)"""
    d = dense != 0
    for _ in range(iters):
        p = np.pad(d, [(0, 0)] * (d.ndim - 2) + [(1, 1), (1, 1)], constant_values=True)
        d = p[..., 1:-1, 1:-1] & p[..., :-2, 1:-1] & p[..., 2:, 1:-1] & p[..., 1:-1, :-2] & p[..., 1:-1, 2:]
    return d


def _words(members, u, v):
    """label words [n, LW] of points at pixels (u, v) from members bool [M,H,W]"""
    M = members.shape[0]
    out = np.zeros((len(u), (M + 31) // 32), np.uint32)
    for m in range(M):
        out[:, m >> 5] |= members[m, v, u].astype(np.uint32) << np.uint32(m & 31)
    return out


def _same(a, b, what="result"):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (what, i))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), what
    else:
        assert a == b, (what, a, b)


def _every_pixel_is_hit(res, W, H, stride=1):
    for f, r in enumerate(res):
        hit = np.zeros((H, W), bool)
        uvv = r["uv_valid"]
        assert len(uvv) == r["n_valid"] and (uvv[:, 0] >= 0).all() and (uvv[:, 0] < W).all() and (uvv[:, 1] >= 0).all() and (uvv[:, 1] < H).all()
        hit[uvv[:, 1], uvv[:, 0]] = True
        assert hit[::stride, ::stride].all(), (f, int((~hit[::stride, ::stride]).sum()))
        assert np.array_equal(r["u"][r["valid_idx"]], uvv[:, 0]) and np.array_equal(r["v"][r["valid_idx"]], uvv[:, 1])


def _words_are_right(res, members):
    """label_words of every frame against the members [F,M,H,W] at the valid points' pixels; no bit on an invalid point"""
    for f, r in enumerate(res):
        vi, uvv = r["valid_idx"], r["uv_valid"]
        want = np.zeros_like(r["label_words"])
        want[vi] = _words(members[f], uvv[:, 0], uvv[:, 1])
        assert np.array_equal(r["label_words"], want), f
        assert np.array_equal(r["label_valid_words"], want[vi]), f


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


def _setup(c, W, H, F, K=None):
    c.set_erosion_element(3)
    c.set_camera(T, _K(W, H) if K is None else K, W, H, 0.0, 50.0)
    c.set_boxes(_boxes(F), oriented=False)


def _both(c, pts, dense, **kw):
    want = c.run_wide(pts, np.ascontiguousarray(dense), **WANT, **kw)
    got = c.run_wide(pts, _rles(dense), **WANT, **kw)
    _same(got, want)
    return got


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", [0, 1, 31, 32, 33, 64, 65, 255, 256])
def test_run_wide_equals_the_dense_call(ctx, M, F):
    for W, H in (SMALL, MID):
        _setup(ctx, W, H, F)
        pts = _cloud(W, H, F)
        dense = _masks(F, M, W, H)
        got = _both(ctx, pts, dense)
        _every_pixel_is_hit(got, W, H)
        _words_are_right(got, dense != 0)
        assert len(got) == F and got[0]["label_words"].shape[1] == (M + 31) // 32
        if M:
            assert all(r["n_labelled"] > 0 and r["count_mb"].shape == (M, 2) for r in got) and (M < 31 or got[0]["count_mb"].any())
            one = ctx.run_wide(pts[:1], _rles(dense)[0], **WANT) if F == 1 else None      # one RleMasks, not a list
            if one is not None:
                _same(one, got)


def test_full_image_run_as_bit_0_of_word_1(ctx):
    """one run that is the whole 1408 x 376 image (517 units) as mask 32, behind 32 empty masks; a sparse cloud"""
    W, H = LARGE
    _setup(ctx, W, H, 1)
    pts = _cloud(W, H, 1, stride=8)
    off = np.zeros(34, np.int64)
    off[33] = 1
    r = RleMasks(np.array([[0, W * H]], np.int32), off, (33, H, W))
    dense = r.to_dense()
    assert dense[32].all() and not dense[:32].any()
    want = ctx.run_wide(pts, dense[None], **WANT)
    got = ctx.run_wide(pts, r, **WANT)
    _same(got, want)
    _every_pixel_is_hit(got, W, H, stride=8)
    lw = got[0]["label_valid_words"]
    assert len(lw) > 8000 and (lw[:, 0] == 0).all() and (lw[:, 1] == 1).all()
    assert got[0]["inst_count"][32] == got[0]["n_valid"] == got[0]["n_labelled"]


def test_256_masks_on_the_same_pixels_decoded_five_times(ctx):
    W, H = SMALL
    _setup(ctx, W, H, 3)
    pts = _cloud(W, H, 3)
    one = _masks(3, 1, W, H)
    one[:, 0].reshape(3, -1)[:, 100:400] = 1
    dense = np.repeat(one, 256, axis=1)
    want = ctx.run_wide(pts, dense, **WANT)
    for _ in range(5):
        _same(ctx.run_wide(pts, _rles(dense), **WANT), want)
    _words_are_right(want, dense != 0)
    inside = want[0]["label_valid_words"][:, 0] != 0
    assert inside.any() and (want[0]["label_valid_words"][inside] == 0xFFFFFFFF).all()


def _scrambled(r, seed):
    """The same members from runs cut into overlapping pieces, with repeats and empty runs, in shuffled order."""
    rng = np.random.default_rng(seed)
    M, H, W = r.shape
    runs, off = [], [0]
    for m in range(M):
        mine = []
        for s, n in r.runs[r.run_off[m]:r.run_off[m + 1]].tolist():
            cut = int(rng.integers(0, n + 1))
            lap = int(rng.integers(0, min(cut, n - cut) + 1))
            mine += [(s, cut), (s + cut - lap, n - cut + lap), (s + int(rng.integers(0, n)), 0)]
            if rng.random() < 0.3:
                mine.append((s, n))
        order = rng.permutation(len(mine))
        runs += [mine[i] for i in order]
        off.append(len(runs))
    return RleMasks(np.array(runs, np.int32).reshape(-1, 2), np.array(off, np.int64), r.shape)


def test_shuffled_overlapping_and_repeated_runs(ctx):
    W, H = MID
    _setup(ctx, W, H, 2)
    pts = _cloud(W, H, 2)
    dense = _masks(2, 65, W, H)
    want = ctx.run_wide(pts, dense, **WANT)
    messy = [_scrambled(r, 5 + i) for i, r in enumerate(_rles(dense))]
    assert all(len(m.runs) > len(r.runs) and np.array_equal(m.to_dense(), d) for m, r, d in zip(messy, _rles(dense), dense))
    _same(ctx.run_wide(pts, messy, **WANT), want)


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("iters", [0, 1, 2])
def test_erosion_runs_on_the_packed_planes(ctx, iters, k):
    for W, H in (SMALL, MID):
        _setup(ctx, W, H, 2)
        ctx.set_erosion_element(k)
        try:
            pts = _cloud(W, H, 2)
            dense = _masks(2, 40, W, H)
            got = _both(ctx, pts, dense, erode_iters=iters)
            _every_pixel_is_hit(got, W, H)
            if k == 3:
                members = _erode_cross(dense, iters)
                _words_are_right(got, members)
                assert members.any() and (iters == 0 or (members != (dense != 0)).any())
        finally:
            ctx.set_erosion_element(3)


def test_pipelined_context_with_a_narrow_run_owed():
    """fused-pack mode: a narrow device run is queued (its tail and summaries ride in later launches), then the wide run-length call:
    it launches what is owed and runs in order.  Both give what a serial context gives"""
    import torch
    W, H = MID
    pts = _cloud(W, H, 1)
    narrow, dense = _masks(1, 5, W, H), _masks(1, 40, W, H)
    dev = torch.device("cuda", 0)
    n = len(pts[0])
    with LpfContext(0) as serial:
        _setup(serial, W, H, 1)
        serial.set_masks_rle(_rles(narrow))
        want_narrow = serial.run_batch(pts, **NARROW)
        want_wide = serial.run_wide(pts, dense, **WANT)
    with LpfContext(0) as c:
        c.set_pipelined("fused-pack")
        _setup(c, W, H, 1)
        tp = torch.from_numpy(pts[0]).to(dev)
        uv = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        bits = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        c.set_masks_rle(_rles(narrow))
        c.run_device(tp, [0, n], uv=uv, label_bits=bits)
        got = c.run_wide(pts, _rles(dense), **WANT)
        c.sync()
        _same(got, want_wide)
        assert np.array_equal(uv.cpu().numpy(), np.stack([want_narrow[0]["u"], want_narrow[0]["v"]], axis=1))
        assert np.array_equal(bits.cpu().numpy().view(np.uint32), want_narrow[0]["label_bits"])
        c.set_pipelined(False)


def test_narrow_state_is_left_as_it_was(ctx):
    W, H = SMALL
    _setup(ctx, W, H, 2)
    pts = _cloud(W, H, 2)
    ctx.set_masks_rle(_rles(_masks(2, 5, W, H)))
    img0 = ctx.get_label_image()
    run0 = ctx.run_batch(pts, **NARROW)
    ctx.run_wide(pts, _rles(_masks(2, 40, W, H)), erode_iters=1, **WANT)
    ctx.run_cams_wide(pts, [dict(T_velo_to_rect=T, K=_K(W, H), width=W, height=H, masks=_rles(_masks(2, 33, W, H)))], **WANT)
    ctx.run_cams(pts, [dict(T_velo_to_rect=T, K=_K(W, H), width=W, height=H, masks=_rles(_masks(2, 9, W, H)))])
    assert np.array_equal(ctx.get_label_image(), img0) and img0.any()
    _same(ctx.run_batch(pts, **NARROW), run0)
    assert (ctx.M, ctx.F_masks) == (5, 2)


def _union_cloud(sizes, F):
    """every pixel of every camera in ``sizes`` ((W, H, K)) is hit: the cameras' clouds, frame by frame"""
    per = [_cloud(W, H, F, K=K) for W, H, K in sizes]
    return [np.ascontiguousarray(np.concatenate([p[f] for p in per])) for f in range(F)]


def test_run_cams_wide_with_cameras_of_different_sizes_and_forms():
    F = 2
    sizes = [SMALL + (_K(*SMALL),), MID + (_K(*MID),), SMALL + (_K(*SMALL, f=30.0),)]
    pts = _union_cloud(sizes, F)
    dense = [_masks(F, 40, *SMALL), _masks(F, 33, *MID), _masks(F, 5, *SMALL)[:, ::-1].copy()]
    erode = [1, 0, 2]
    boxes = _boxes(F)
    cams = [dict(T_velo_to_rect=T, K=K, width=W, height=H, erode_iters=e, boxes=boxes, oriented=False, masks=(d if k == 1 else _rles(d)))
            for k, ((W, H, K), d, e) in enumerate(zip(sizes, dense, erode))]
    with LpfContext(0) as c:
        got = c.run_cams_wide(pts, cams, **WANT)
    for k, ((W, H, K), d, e) in enumerate(zip(sizes, dense, erode)):
        with LpfContext(0) as fresh:
            fresh.set_camera(T, K, W, H, 0.0, 50.0)
            fresh.set_boxes(boxes, oriented=False)
            want = fresh.run_wide(pts, d, erode_iters=e, **WANT)
        _same(got[k], want, "camera %d" % k)
        _every_pixel_is_hit(got[k], W, H)
        _words_are_right(got[k], _erode_cross(d, e))
        assert got[k][0]["n_labelled"] > 0


@pytest.mark.parametrize("case", ["rle 9 + float 20", "all narrow", "all narrow, 5 x 5 element"])
def test_run_cams_beside_dense_and_at_one_byte_labels(case):
    F = 2
    element = 5 if case.endswith("5 x 5 element") else 3          # the erosion element, on the pass's context and on the yardstick's
    boxes = _boxes(F)
    if case == "rle 9 + float 20":
        sizes = [SMALL + (_K(*SMALL),), MID + (_K(*MID),)]
        dense = [_masks(F, 9, *SMALL), _masks(F, 20, *MID).astype(np.float32)]
        erode, forms = [1, 0], ["rle", "dense"]
    else:                                                    # M <= 8 everywhere: one-byte label elements on the 851-pixel image
        sizes = [SMALL + (_K(*SMALL),), SMALL + (_K(*SMALL, f=30.0),)]
        dense = [_masks(F, 8, *SMALL), _masks(F, 3, *SMALL)[:, ::-1].copy()]
        erode, forms = [0, 2], ["rle", "rle"]
    pts = _union_cloud(sizes, F)
    cams = [dict(T_velo_to_rect=T, K=K, width=W, height=H, erode_iters=e, boxes=boxes, oriented=False,
                 masks=_rles(d) if form == "rle" else d) for (W, H, K), d, e, form in zip(sizes, dense, erode, forms)]
    with LpfContext(0) as c:
        c.set_erosion_element(element)
        try:
            got = c.run_cams(pts, cams, **NARROW)
        finally:
            c.set_erosion_element(3)
    for k, ((W, H, K), d, e) in enumerate(zip(sizes, dense, erode)):
        with LpfContext(0) as fresh:
            fresh.set_erosion_element(element)
            try:
                fresh.set_camera(T, K, W, H, 0.0, 50.0)
                fresh.set_masks(np.ascontiguousarray(d), erode_iters=e)
                fresh.set_boxes(boxes, oriented=False)
                want = fresh.run_batch(pts, **NARROW)
            finally:
                fresh.set_erosion_element(3)
        _same(got[k], want, "camera %d" % k)
        _every_pixel_is_hit(got[k], W, H)
        if element == 3:
            members = _erode_cross(d, e)
            for f, r in enumerate(got[k]):
                uvv = r["uv_valid"]
                assert np.array_equal(r["label_valid"], _words(members[f], uvv[:, 0], uvv[:, 1])[:, 0]), (k, f)
        assert got[k][0]["n_labelled"] > 0


def _camera(W, H):
    return kitti360.CameraPerspective.from_arrays(_K(W, H), np.eye(3), W, H)


def _same_frames(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in sorted(a):
        x, y = a[key], b[key]
        if key == "car_statistics":
            assert x == y, (what, key)
        elif isinstance(x, list):
            assert len(x) == len(y) and all(np.array_equal(p, q) and np.asarray(p).dtype == np.asarray(q).dtype for p, q in zip(x, y)), (what, key)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), (what, key)
        else:
            assert x == y, (what, key)


def _frame_inputs(pts, masks, boxes):
    return [pipeline.FrameInputs(100 + i, p, m, [{"corners_velo": c.tolist()} for c in b]) for i, (p, m, b) in enumerate(zip(pts, masks, boxes))]


class _Counted:
    """ctx.run_wide and ctx.set_masks_rle counted, RleMasks.to_dense raising, while in the with block"""
    def __init__(self, monkeypatch, c):
        self.calls = dict(run_wide=0, set_masks_rle=0)
        for name in self.calls:
            def counted(*a, _name=name, _fn=getattr(c, name), **kw):
                self.calls[_name] += 1
                return _fn(*a, **kw)
            monkeypatch.setattr(c, name, counted)

        def no_dense(self_):
            raise AssertionError("RleMasks.to_dense was called: the runs must reach the GPU as runs")
        monkeypatch.setattr(RleMasks, "to_dense", no_dense)


def test_run_frames_takes_33_to_256_rle_masks_in_one_wide_pass(monkeypatch):
    W, H = MID
    pts = _cloud(W, H, 2)
    boxes = _boxes(2)
    cam = _camera(W, H)
    with LpfContext(0) as c:
        for dense in ([_masks(1, 40, W, H)[0], _masks(2, 7, W, H)[1]], [_masks(1, 256, W, H)[0], _masks(2, 40, W, H)[1]]):
            want = pipeline.run_frames(_frame_inputs(pts, dense, boxes), T, cam, 50.0, 10, False, ctx=c)
            rles = _rles(dense)
            with monkeypatch.context() as mp:
                counted = _Counted(mp, c)
                got = pipeline.run_frames(_frame_inputs(pts, rles, boxes), T, cam, 50.0, 10, False, ctx=c)
                for i, (a, b) in enumerate(zip(got, want)):
                    _same_frames(a, b, "frame %d" % i)       # (the lazy keys are gathered here, still without to_dense)
            assert counted.calls == dict(run_wide=1, set_masks_rle=0)
            assert len(got) == 2 and len(got[0]["car_point_sets"]) == len(dense[0]) and got[0]["bg_assigned"].any()


def test_run_frames_runs_300_rle_masks_in_two_groups(monkeypatch):
    W, H = SMALL
    pts = _cloud(W, H, 1)
    boxes = _boxes(1)
    cam = _camera(W, H)
    dense = [np.concatenate([_masks(1, 256, W, H)[0], _masks(2, 44, W, H)[1]])]
    assert dense[0].shape[0] == 300
    with LpfContext(0) as c:
        want = pipeline.run_frames(_frame_inputs(pts, dense, boxes), T, cam, 50.0, 10, False, ctx=c)
        rles = _rles(dense)
        with monkeypatch.context() as mp:
            counted = _Counted(mp, c)
            got = pipeline.run_frames(_frame_inputs(pts, rles, boxes), T, cam, 50.0, 10, False, ctx=c)
            _same_frames(got[0], want[0], "300 masks")
        assert counted.calls == dict(run_wide=2, set_masks_rle=0)
        assert len(got[0]["car_point_sets"]) == 300


def test_run_frames_multicam_takes_rle_frames():
    """camera 0: RleMasks, 9 and 4 masks (the pass); camera 1: dense, 5 masks (the same pass); camera 2: RleMasks, 40 masks (run_frames)"""
    F = 2
    sizes = [SMALL, MID, SMALL]
    cams = [(T, _camera(W, H)) for W, H in sizes]
    pts = _union_cloud([s + (_K(*s),) for s in sizes[:2]], F)
    boxes = _boxes(F)
    dense = [[_masks(1, 9, *SMALL)[0], _masks(2, 4, *SMALL)[1]], [_masks(1, 5, *MID)[0], _masks(2, 5, *MID)[1]],
             [_masks(1, 40, *SMALL)[0], _masks(2, 33, *SMALL)[1]]]
    given = [_rles(dense[0]), dense[1], _rles(dense[2])]
    with LpfContext(0) as c:
        got = pipeline.run_frames_multicam([_frame_inputs(pts, m, boxes) for m in given], cams, 50.0, 10, False, erode_iters=1, ctx=c)
        for k in range(3):
            for form, masks in (("same form", given[k]), ("dense", dense[k])):
                want = pipeline.run_frames(_frame_inputs(pts, masks, boxes), T, cams[k][1], 50.0, 10, False, erode_iters=1, ctx=c)
                for i, (a, b) in enumerate(zip(got[k], want)):
                    _same_frames(a, b, "camera %d frame %d against %s" % (k, i, form))
            assert got[k][0]["bg_assigned"].any()
