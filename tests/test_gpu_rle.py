"""lpf_set_masks_rle on the GPU: after run-length masks are set the context is in the state the equivalent dense uint8 host masks
leave -- the label image bit for bit (all three element widths, byte lanes that straddle words, a partial last word, 32 masks on the
same pixels, a run that is the whole image, runs shuffled and overlapping, erosion with the cross and the 5 x 5 element), every output
of the runs that follow (in order, through lpf_run_frame, in the pipelined modes), across a sequence of calls that changes form and
width, and through pipeline.run_frames.  The dense path is the yardstick, held against NumPy and the CPU oracle where that is cheap."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden, unpack_masks
from lidar_object_detection_amd import kitti360, pipeline
from lidar_object_detection_amd._native import LpfContext, LpfError, RleMasksInput, SUMMARY_DTYPE
from lidar_object_detection_amd.rle import RleMasks
from oracle import cpu_oracle as orc

pytestmark = pytest.mark.gpu

SMALL, LARGE = (37, 23), (1408, 376)        # W x H: 851 pixels (no multiple of 4: a partial last word) / the real camera
ALL = dict(want_uv=True, want_label=True, want_float=True, want_lists=True, want_valid_uv=True)


@pytest.fixture(scope="module")
def ctx():
    c = LpfContext(0)
    yield c
    c.close()


def _camera(c, calib, W, H, dmax=50.0):
    """the calibration's camera scaled to a W x H image"""
    K = np.diag([W / float(calib["width"]), H / float(calib["height"]), 1.0]) @ np.asarray(calib["K"], np.float64)[:3, :3]
    c.set_camera(calib["TrVeloToRect"], K, W, H, 0.0, dmax)
    return K


_base = {}


def _masks(F, M, W, H):
    """uint8 0 / 1 [F,M,H,W], the same for every caller: rectangles, disks, sparse noise inside a rectangle, some masks empty (ragged run
    counts), overlaps between masks"""
    if (W, H) not in _base:
        rng = np.random.default_rng(W * 1000 + H)
        yy, xx = np.mgrid[:H, :W]
        b = np.zeros((3, 32, H, W), np.uint8)
        for f in range(3):
            for m in range(32):
                cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.1, 0.45) * H
                kind = (m + f) % 4
                if kind == 0:
                    b[f, m] = (abs(yy - cy) <= r) & (abs(xx - cx) <= 2 * r)
                elif kind == 1:
                    b[f, m] = (yy - cy) ** 2 + ((xx - cx) / 2.0) ** 2 <= r * r
                elif kind == 2:
                    b[f, m] = (abs(yy - cy) <= r) & (abs(xx - cx) <= r) & (rng.random((H, W)) < 0.3)
                # kind 3: an empty mask
        b[0, 0, 0, 0] = b[0, 0, H - 1, W - 1] = 1            # the first and the last pixel of an image
        b[2, 1, H - 1, W - 3:] = 1                           # ... and of the batch
        _base[(W, H)] = b
    return _base[(W, H)][:F, :M]


def _label(dense):
    """[F,M,H,W] members -> uint32 [F,H,W], bit m = mask m"""
    out = np.zeros(dense.shape[:1] + dense.shape[2:], np.uint32)
    for m in range(dense.shape[1]):
        out |= (dense[:, m] != 0).astype(np.uint32) << np.uint32(m)
    return out


def _rles(dense):
    return [RleMasks.from_dense(d) for d in dense]


def _dense_image(c, dense, erode_iters=0):
    c.set_masks(np.ascontiguousarray(dense), erode_iters=erode_iters)
    return c.get_label_image()


def _rle_image(c, rles, erode_iters=0):
    c.set_masks_rle(rles, erode_iters=erode_iters)
    return c.get_label_image()


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


@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("M", [0, 1, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("cam", [SMALL, LARGE], ids=["37x23", "1408x376"])
def test_label_image_equals_the_dense_path(ctx, calib, cam, M, F):
    W, H = cam
    _camera(ctx, calib, W, H)
    dense = _masks(F, M, W, H)
    want = _dense_image(ctx, dense)
    got = _rle_image(ctx, _rles(dense))
    assert got.shape == (F, H, W) and np.array_equal(got, want)
    assert np.array_equal(want, _label(dense)) and (want.any() or M == 0)
    assert ctx.M == M and ctx.F_masks == F


def test_label_image_of_the_edge_shapes(ctx, calib):
    W, H = SMALL
    _camera(ctx, calib, W, H)
    z = np.zeros((H, W), np.uint8)
    full = np.ones((H, W), np.uint8)
    first, last, cross = z.copy(), z.copy(), z.copy()
    first[0, 0] = last[H - 1, W - 1] = 1
    cross[3, W - 4:] = cross[4, :5] = 1
    yy, xx = np.mgrid[:H, :W]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    shapes = np.stack([z, full, first, last, cross, board])
    for reps in (1, 2, 4):                                   # 6, 12, 24 masks: 1-, 2- and 4-byte label elements
        dense = np.concatenate([shapes] * reps)[None]
        dense = np.concatenate([dense, dense[:, ::-1]])      # two frames: frame 1 begins in the middle of a word
        want = _dense_image(ctx, dense)
        assert np.array_equal(_rle_image(ctx, _rles(dense)), want) and np.array_equal(want, _label(dense))


def test_one_run_that_is_the_whole_image(ctx, calib):
    W, H = LARGE
    _camera(ctx, calib, W, H)
    for M, m in [(3, 1), (12, 11), (32, 31)]:
        off = np.zeros(M + 1, np.int64)
        off[m + 1:] = 1
        r = RleMasks(np.array([[0, W * H]], np.int32), off, (M, H, W))
        got = _rle_image(ctx, r)
        assert got.shape == (1, H, W) and (got == np.uint32(1 << m)).all()
        dense = np.zeros((1, M, H, W), np.uint8)
        dense[0, m] = 1
        assert np.array_equal(got, _dense_image(ctx, dense))


def test_32_masks_on_the_same_pixels_decode_identically_every_time(ctx, calib):
    """OR contention: every word of the members is hit by 32 waves.  Integer ORs only -- the image cannot depend on their order."""
    W, H = LARGE
    _camera(ctx, calib, W, H)
    one = _masks(1, 3, W, H)[0]
    one = (one[0] | one[1] | one[2])[None]
    dense = np.repeat(one, 32, axis=0)[None]
    rles = _rles(dense)
    want = _dense_image(ctx, dense)
    assert set(np.unique(want).tolist()) == {0, 0xFFFFFFFF}
    images = [_rle_image(ctx, rles) for _ in range(5)]
    for img in images:
        assert np.array_equal(img, want)
    for M in (8, 16):                                        # the same contention inside one word's byte and half-word lanes
        assert np.array_equal(_rle_image(ctx, [rles[0][:M]]), _dense_image(ctx, dense[:, :M]))


@pytest.mark.parametrize("cam", [SMALL, LARGE], ids=["37x23", "1408x376"])
def test_runs_shuffled_and_overlapping(ctx, calib, cam):
    W, H = cam
    _camera(ctx, calib, W, H)
    for M in (7, 13, 20):
        dense = _masks(2, M, W, H)
        canon = _rles(dense)
        odd = [_scrambled(r, 40 + M + f) for f, r in enumerate(canon)]
        assert all(len(o.runs) > 2 * len(r.runs) and np.array_equal(o.to_dense(), r.to_dense()) for o, r in zip(odd, canon))
        assert np.array_equal(_rle_image(ctx, odd), _dense_image(ctx, dense))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("cam", [SMALL, LARGE], ids=["37x23", "1408x376"])
def test_erosion_equals_the_dense_path(ctx, calib, cam, k):
    W, H = cam
    _camera(ctx, calib, W, H)
    ctx.set_erosion_element(k)
    try:
        for M in (5, 9, 20):
            dense = _masks(2, M, W, H)
            rles = _rles(dense)
            plain = _dense_image(ctx, dense, 0)
            seen = [plain]
            for iters in (0, 1, 2):
                want = _dense_image(ctx, dense, iters)
                assert np.array_equal(_rle_image(ctx, rles, iters), want), (M, iters)
                seen.append(want)
            assert seen[2].any() and not np.array_equal(seen[2], plain) and not np.array_equal(seen[3], seen[2])    # not vacuous
    finally:
        ctx.set_erosion_element(3)


def test_a_refused_call_leaves_the_context_as_it_was(ctx, calib):
    W, H = SMALL
    _camera(ctx, calib, W, H)
    dense = _masks(2, 9, W, H)
    want = _rle_image(ctx, _rles(dense))
    bad = _rles(dense[:1, :3])[0]
    runs, run_off, F, M = ctx.rle_batch(bad, H, W)
    runs = runs.copy()
    runs[len(runs) // 2] = (W * H - 1, 2)                    # one pixel past the image: past the Python checks, straight to the library
    s = RleMasksInput(runs.ctypes.data, run_off.ctypes.data, F, M, 0, 0)
    rc = ctx._lib.lpf_set_masks_rle(ctx._h, ctypes.byref(s))
    with pytest.raises(LpfError, match=r"frame 0 mask \d run \d+: start=850 length=2"):
        ctx._check(rc)
    assert ctx.M == 9 and ctx.F_masks == 2 and np.array_equal(ctx.get_label_image(), want)


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


def _cam(calib):
    return kitti360.CameraPerspective.from_arrays(calib["K"], calib["R_rect"], int(calib["width"]), int(calib["height"]))


_golden = {}


def _frame100(calib):
    """golden frame 100 (subsampled): points, boxes, its five synthetic masks dense and as runs, and the CPU oracle's result -- once"""
    if not _golden:
        g = load_golden(100)
        W, H = int(calib["width"]), int(calib["height"])
        dense = (unpack_masks(g, "rect5", H, W) != 0).astype(np.uint8)
        T, K = calib["TrVeloToRect"], np.asarray(calib["K"], np.float64)[:3, :3]
        ref = orc.run(g["points"], T, K, W, H, 0.0, 50.0, label_img=orc.pack_masks(dense, 0, H, W), M=5, corners=g["corners_velo"], oriented=True)
        _golden.update(points=g["points"], corners=np.asarray(g["corners_velo"], np.float64), dense=dense, rle=RleMasks.from_dense(dense),
                       T=T, K=K, W=W, H=H, ref=ref)
        assert ref["inst_count"].sum() > 0 and ref["count_mb"].any()
    return _golden


def _equals_oracle(r, ref):
    assert r["n_valid"] == ref["n_valid"] and np.array_equal(r["valid_idx"], ref["valid_idx"])
    assert np.array_equal(r["u"], ref["u"]) and np.array_equal(r["v"], ref["v"]) and np.array_equal(r["label_bits"], ref["label_bits"])
    for k in ("depth", "uf", "vf"):
        assert r[k].tobytes() == ref[k].tobytes(), k
    assert np.array_equal(r["inst_count"], ref["inst_count"]) and np.array_equal(r["count_mb"], ref["count_mb"])
    assert all(np.array_equal(a, b) for a, b in zip(r["inst_lists"], ref["inst_lists"])) and len(r["inst_lists"]) == len(ref["inst_lists"])
    assert np.array_equal(r["best_cnt"], ref["best_cnt"]) and np.array_equal(r["best_box"], ref["best_box"])


@pytest.mark.parametrize("mode", [False, "fused", "fused-pack"])
def test_golden_frame_every_output_equals_dense_and_oracle(calib, mode):
    """run_batch after set_masks_rle: in order one run, in the pipelined modes (2 / 4) three consecutive runs with the masks set before
    each, as those modes ask"""
    G = _frame100(calib)
    with LpfContext(0) as c:
        c.set_pipelined(mode)
        c.set_camera(G["T"], G["K"], G["W"], G["H"], 0.0, 50.0)
        c.set_boxes([G["corners"]], oriented=True)
        for it in range(3 if mode else 1):
            c.set_masks(G["dense"][None])
            want = c.run_batch([G["points"]], **ALL)
            c.set_masks_rle(G["rle"])
            got = c.run_batch([G["points"]], **ALL)
            c.sync()
            _same(got, want, "run_batch %s %d" % (mode, it))
            _equals_oracle(got[0], G["ref"])
        three = [c.set_masks_rle(G["rle"]) or c.run_batch([G["points"]], **ALL) for _ in range(3)]      # rle only, back to back
        c.sync()
        for r in three:
            _equals_oracle(r[0], G["ref"])


def test_golden_frame_through_run_frame_with_the_masks_in_force(calib):
    """lpf_run_frame with masks == NULL runs with the masks lpf_set_masks_rle left in force"""
    import torch
    G = _frame100(calib)
    dev = torch.device("cuda", 0)
    n, M, B = len(G["points"]), 5, len(G["corners"])
    pts = torch.from_numpy(G["points"]).to(dev)

    def outs():
        return dict(uv=torch.zeros((n, 2), dtype=torch.int32, device=dev), label_bits=torch.zeros(n, dtype=torch.int32, device=dev),
                    valid_idx=torch.zeros(n, dtype=torch.int64, device=dev), inst_idx=torch.zeros(n, dtype=torch.int64, device=dev),
                    inst_cap=n, count_mb=torch.zeros(M * B, dtype=torch.int32, device=dev),
                    summary=torch.zeros(SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev))
    results = []
    with LpfContext(0) as c:
        c.set_camera(G["T"], G["K"], G["W"], G["H"], 0.0, 50.0)
        c.set_boxes([G["corners"]], oriented=True)
        for form in ("dense", "rle"):
            o = outs()
            torch.cuda.synchronize()
            if form == "dense":
                c.set_masks(G["dense"][None])
            else:
                c.set_masks_rle(G["rle"])
            c.make_frame_step(pts, **o)()
            c.sync()
            results.append({k: v.cpu().numpy() for k, v in o.items() if k != "inst_cap"})
    _same(results[1], results[0], "lpf_run_frame")
    ref, r = G["ref"], results[1]
    summ = r["summary"].view(SUMMARY_DTYPE)[0]
    nv = int(summ["n_valid"])
    assert nv == ref["n_valid"] and np.array_equal(r["valid_idx"][:nv], ref["valid_idx"])
    assert np.array_equal(r["label_bits"].view(np.uint32), ref["label_bits"])
    assert np.array_equal(r["uv"][:, 0], ref["u"]) and np.array_equal(r["uv"][:, 1], ref["v"])
    assert np.array_equal(summ["inst_count"][:M], ref["inst_count"]) and np.array_equal(r["count_mb"].reshape(M, B), ref["count_mb"])


def test_state_sequence_equals_its_dense_twin(calib):
    """rle (M = 5) -> run -> dense u8 -> run -> rle (M = 20: the label width changes) -> run -> set_mask_rects + rle (the hint is consumed
    and ignored) -> run -> dense u8 (it must not see that hint) -> run; a twin context gets the same masks dense every time"""
    W, H = 300, 80
    g = load_golden(100)
    m5, m20 = _masks(1, 5, W, H), _masks(2, 20, W, H)[1:]
    other = _masks(3, 7, W, H)[2:]
    wrong = np.zeros((1, 5, 4), np.int32)
    wrong[..., 2:] = 3                                       # 3 x 3 rectangles: they do NOT hold, so using them would show
    steps = [("rle", m5, None), ("dense", other, None), ("rle", m20, None), ("rle", m5, wrong), ("dense", m5, None)]
    with LpfContext(0) as c, LpfContext(0) as twin:
        for x in (c, twin):
            _camera(x, calib, W, H)
            x.set_boxes([np.asarray(g["corners_velo"], np.float64)], oriented=True)
        for i, (form, dense, rects) in enumerate(steps):
            if rects is not None:
                c.set_mask_rects(rects)
            if form == "rle":
                c.set_masks_rle(_rles(dense))
            else:
                c.set_masks(np.ascontiguousarray(dense))
            twin.set_masks(np.ascontiguousarray(dense))
            got, want = c.run_batch([g["points"]], **ALL), twin.run_batch([g["points"]], **ALL)
            assert want[0]["n_labelled"] > 0, i
            _same(got, want, "step %d" % i)
            assert np.array_equal(c.get_label_image(), _label(dense)), i


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


@pytest.mark.parametrize("case", ["M=5", "M=40", "erode+v3"])
def test_run_frames_takes_rle_frames(calib, case):
    """pipeline.run_frames with RleMasks frames against the same frames dense, FrameResult key for key: one narrow pass, two groups of
    32 (the dense twin takes the wide pass), and erode_iters = 1 with v3_pipeline"""
    G = _frame100(calib)
    cam = _cam(calib)
    W, H = G["W"], G["H"]
    boxes = [{"corners_velo": c.tolist()} for c in G["corners"]]
    if case == "M=40":
        dense = [np.concatenate([_masks(1, 32, W, H)[0], _masks(2, 8, W, H)[1]]), G["dense"]]       # ragged: 40 and 5
    else:
        dense = [G["dense"], _masks(1, 3, W, H)[0]]
    kw = dict(erode_iters=1, v3_pipeline=True) if case == "erode+v3" else {}
    pts = [G["points"], G["points"][::2]]

    def run(masks):
        return pipeline.run_frames([pipeline.FrameInputs(100 + i, p, m, boxes) for i, (p, m) in enumerate(zip(pts, masks))],
                                   G["T"], cam, 50.0, 10, True, **kw)
    want = run(dense)
    got = run([RleMasks.from_dense(d) for d in dense])
    assert len(got) == len(want) == 2
    for i, (a, b) in enumerate(zip(got, want)):
        _same_frames(a, b, "%s frame %d" % (case, i))
    assert any(d["total_points"] for d in got[0]["car_statistics"]) and len(got[0]["car_point_sets"]) == len(dense[0])
    # a frame without masks in a batch of RleMasks frames counts as no masks
    if case == "M=5":
        mixed = pipeline.run_frames([pipeline.FrameInputs(100, pts[0], RleMasks.from_dense(dense[0]), boxes), pipeline.FrameInputs(2, pts[1], None, boxes),
                                     pipeline.FrameInputs(3, pts[1], [], boxes)], G["T"], cam, 50.0, 10, True)
        _same_frames(mixed[0], want[0], "with maskless frames")
        assert len(mixed[1]["car_point_sets"]) == 0 and not mixed[2]["bg_assigned"].any()
