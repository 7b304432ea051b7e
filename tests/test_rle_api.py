"""Run-length masks (lpf_set_masks_rle, rle.RleMasks) without a GPU: the header declares the struct and the call, the ctypes mirror
matches the C layout, the library exports the entry point and carries the decode kernel, RleMasks agrees with the independent NumPy
restatement of tests/rle_ref.py, and the Python entries refuse bad input before anything reaches the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rle_ref as R
from conftest import golden_frames, load_golden, unpack_masks
from lidar_object_detection_amd import _build, _native, pipeline
from lidar_object_detection_amd._native import RleMasksInput
from lidar_object_detection_amd.rle import RleMasks
from test_wide_api import HEADER, _NoGpu, _c_layout, _header_text


def test_header_declares_the_struct_and_the_call():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert re.search(r"\bint\s+lpf_set_masks_rle\s*\(\s*lpf_ctx\s*\*\s*\w*\s*,\s*const\s+lpf_rle_masks\s*\*\s*\w*\s*\)", text)
    assert re.search(r"typedef\s+struct\s+lpf_rle_masks\s*\{", text) and re.search(r"\}\s*lpf_rle_masks\s*;", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", _header_text())
    assert "8 (continued): lpf_rle_masks, lpf_set_masks_rle (added; nothing else changed)" in _header_text()
    assert "lpf_set_masks_rle" in _native.EXPORTED
    assert "lpf_rle.hip.h" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "lpf_rle.hip.h"))
    assert os.path.isfile(HEADER)


def test_struct_mirror_matches_the_header(tmp_path):
    names = [f[0] for f in RleMasksInput._fields_]
    lay = _c_layout(tmp_path, "lpf_rle_masks", names)
    assert lay["sizeof"] == ctypes.sizeof(RleMasksInput) == 32
    for n in names:
        assert lay[n] == getattr(RleMasksInput, n).offset, n


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_carries_the_entry_point_and_the_decode_kernel():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT lpf_set_masks_rle\b", dyn)
    # (the host stubs of the kernel's three instantiations: uint8, uint16 and uint32 label elements)
    syms = subprocess.run(["nm", _build.LIB], check=True, capture_output=True, text=True).stdout
    for lt in ("IhE", "ItE", "IjE"):
        assert re.search(r"lpf_rle_decode%s" % lt, syms), lt


def _check_against_ref(masks, fast=False):
    masks = np.asarray(masks)
    M, H, W = masks.shape
    r = RleMasks.from_dense(masks)
    assert r.shape == (M, H, W) and len(r) == M
    assert r.runs.dtype == np.int32 and r.runs.shape[1:] == (2,) and r.run_off.dtype == np.int64 and r.run_off.shape == (M + 1,)
    to_runs = R.dense_to_runs_fast if fast else R.dense_to_runs
    for m in range(M):
        got = [tuple(int(v) for v in row) for row in r.runs[r.run_off[m]:r.run_off[m + 1]]]
        assert got == to_runs(masks[m]), m                   # canonical: ascending and maximal
    want = (masks != 0).astype(np.uint8)
    dense = r.to_dense()
    assert dense.dtype == np.uint8 and np.array_equal(dense, want)
    assert np.array_equal(R.masks_to_dense(r.runs, r.run_off, M, H, W), want)
    return r


@pytest.mark.parametrize("H,W,fast", [(23, 37, False), (376, 1408, True)])
def test_from_dense_on_seeded_random_masks(H, W, fast):
    rng = np.random.default_rng(H * W)
    m = np.zeros((4, H, W), np.uint8)
    m[0] = rng.random((H, W)) < 0.5                           # noise: runs of a pixel or two
    m[1] = rng.random((H, W)) < 0.02
    yy, xx = np.mgrid[:H, :W]
    m[2] = (yy - H * 0.4) ** 2 + ((xx - W * 0.6) / 2.0) ** 2 <= (0.3 * H) ** 2      # a blob: one run per row
    m[3] = (m[2] != 0) & (rng.random((H, W)) < 0.97)
    r = _check_against_ref(m * np.uint8(255), fast)
    assert len(r.runs) > 2 * H
    if not fast:
        assert R.dense_to_runs_fast(m[0]) == R.dense_to_runs(m[0])     # the two restatements agree with each other


def test_from_dense_edge_shapes():
    H, W = 23, 37
    z = np.zeros((1, H, W), np.uint8)
    assert len(_check_against_ref(z).runs) == 0                                  # an empty mask
    full = _check_against_ref(np.ones((1, H, W), np.uint8))                      # a full mask: ONE run
    assert full.runs.tolist() == [[0, H * W]]
    first, last = z.copy(), z.copy()
    first[0, 0, 0] = 1
    last[0, H - 1, W - 1] = 7
    assert _check_against_ref(first).runs.tolist() == [[0, 1]]
    assert _check_against_ref(last).runs.tolist() == [[H * W - 1, 1]]
    cross = z.copy()
    cross[0, 3, W - 4:] = 1                                                      # a run that crosses a row end
    cross[0, 4, :5] = 1
    assert _check_against_ref(cross).runs.tolist() == [[3 * W + W - 4, 9]]
    yy, xx = np.mgrid[:H, :W]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)[None]                          # a checkerboard: the most runs (W odd: rows join up)
    assert len(_check_against_ref(board).runs) >= H * W // 2 - H
    assert len(_check_against_ref(np.zeros((0, H, W), np.uint8))) == 0          # no masks at all
    both = _check_against_ref(np.concatenate([first, z, full.to_dense(), last]))
    assert both.run_off.tolist() == [0, 1, 1, 2, 3]


def test_from_dense_rules():
    f = np.array([[[0.0, 0.4, 0.5, 0.6, 1.0, 2.5]]], np.float32)
    assert RleMasks.from_dense(f).runs.tolist() == [[1, 5]]                      # nonzero
    assert RleMasks.from_dense(f, rule="gt0.5").runs.tolist() == [[3, 3]]        # Same_color.py:125
    assert RleMasks.from_dense(f > 0.5).runs.tolist() == [[3, 3]]                # bool
    with pytest.raises(ValueError):
        RleMasks.from_dense(f.astype(np.uint8), rule="gt0.5")
    with pytest.raises(ValueError):
        RleMasks.from_dense(f, rule="round")
    with pytest.raises(ValueError):
        RleMasks.from_dense(f[0])


def test_from_dense_on_the_golden_frames_synthetic_masks(calib):
    H, W = int(calib["height"]), int(calib["width"])
    for entry in golden_frames()["frames"][:4]:
        g = load_golden(int(entry["frame"]))
        for kind in ("rect5", "edge"):
            m = unpack_masks(g, kind, H, W)
            assert m.shape == (entry["n_masks_" + kind], H, W)
            _check_against_ref(m, fast=True)


def test_from_coco_hand_worked():
    # rows 0110 / 0100 / 0001, column-major: 0 0 0 | 1 1 0 | 1 0 0 | 0 0 1 -> 3 zeros, 2 ones, 1 zero, 1 one, 4 zeros, 1 one
    mask = np.array([[0, 1, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.uint8)
    counts = [3, 2, 1, 1, 4, 1]
    assert R.dense_to_coco_counts(mask) == counts and np.array_equal(R.coco_counts_to_dense(counts, 3, 4), mask)
    r = RleMasks.from_coco([counts], 3, 4)
    assert r.shape == (1, 3, 4) and r.runs.tolist() == [[1, 2], [5, 1], [11, 1]] and r.run_off.tolist() == [0, 3]
    assert np.array_equal(r.to_dense()[0], mask)
    # a mask that begins with a one has a leading zero count; an empty and a full mask
    r = RleMasks.from_coco([[0, 12], [12], counts], 3, 4)
    assert r.runs.tolist() == [[0, 12], [1, 2], [5, 1], [11, 1]] and r.run_off.tolist() == [0, 1, 1, 4]
    rng = np.random.default_rng(5)
    m = (rng.random((3, 23, 37)) < 0.3).astype(np.uint8)
    r = RleMasks.from_coco([R.dense_to_coco_counts(p) for p in m], 23, 37)
    assert np.array_equal(r.to_dense(), m)
    with pytest.raises(ValueError):
        RleMasks.from_coco([[3, 2, 1]], 3, 4)                # does not sum to H * W
    with pytest.raises(ValueError):
        RleMasks.from_coco([[13, -1]], 3, 4)


def test_slicing_len_and_shape():
    rng = np.random.default_rng(11)
    m = (rng.random((7, 23, 37)) < 0.2).astype(np.uint8)
    m[3] = 0
    r = RleMasks.from_dense(m)
    assert len(r) == 7 and r.shape == (7, 23, 37)
    for a, b in [(0, 7), (2, 5), (3, 4), (5, 5), (6, 100), (-2, None), (None, 3)]:
        s = r[a:b]
        assert isinstance(s, RleMasks) and s.shape == m[a:b].shape and len(s) == len(m[a:b])
        assert s.run_off[0] == 0 and s.run_off[-1] == len(s.runs)
        assert np.array_equal(s.to_dense(), m[a:b]), (a, b)
    with pytest.raises(TypeError):
        r[2]
    with pytest.raises(TypeError):
        r[::2]


def test_an_rle_never_becomes_an_object_array():
    r = RleMasks.from_dense(np.ones((2, 4, 5), np.uint8))
    with pytest.raises(TypeError, match="to_dense"):
        np.asarray(r)
    with pytest.raises(TypeError, match="to_dense"):
        np.array(r)


def test_rle_constructor_checks_the_runs():
    ok = RleMasks(np.array([[0, 3], [5, 0]], np.int32), np.array([0, 2]), (1, 2, 4))
    assert ok.runs.dtype == np.int32 and ok.run_off.dtype == np.int64
    for runs, off in [(np.array([[-1, 3]], np.int32), [0, 1]), (np.array([[0, -3]], np.int32), [0, 1]), (np.array([[6, 3]], np.int32), [0, 1]),
                      (np.array([[0, 3]], np.float32), [0, 1]), (np.array([0, 3], np.int32), [0, 1]), (np.array([[0, 3]], np.int32), [1, 1]),
                      (np.array([[0, 3]], np.int32), [0, 2]), (np.array([[0, 3]], np.int32), [0, 1, 1]),
                      (np.array([[2 ** 31 - 1, 2 ** 31 - 1]], np.int64), [0, 1])]:
        with pytest.raises(ValueError):
            RleMasks(runs, np.asarray(off), (1, 2, 4))


def _rle(M, H=48, W=64, seed=0):
    return RleMasks.from_dense((np.random.default_rng(seed).random((M, H, W)) < 0.1).astype(np.uint8))


def test_rle_batch_pads_ragged_frames():
    a, b, c = _rle(3, seed=1), _rle(0), _rle(5, seed=2)
    runs, off, F, M = _native.LpfContext.rle_batch([a, b, c], 48, 64)
    assert (F, M) == (3, 5) and runs.dtype == np.int32 and off.dtype == np.int64 and off.shape == (16,)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] == len(runs) == len(a.runs) + len(c.runs)
    dense = np.stack([R.masks_to_dense(runs, off[f * M:(f + 1) * M + 1], M, 48, 64) for f in range(F)])
    want = np.zeros((3, 5, 48, 64), np.uint8)
    want[0, :3], want[2] = a.to_dense(), c.to_dense()
    assert np.array_equal(dense, want)
    one = _native.LpfContext.rle_batch(a, 48, 64)
    assert one[2:] == (1, 3) and np.array_equal(one[0], a.runs) and np.array_equal(one[1], a.run_off)


def _spoiled(field, value):
    r = _rle(2)
    setattr(r, field, value)
    return r


@pytest.mark.parametrize("what", ["wrong size", "33 masks", "start < 0", "length < 0", "past the image", "float runs", "flat runs",
                                  "offsets", "dense", "erode_iters"])
def test_set_masks_rle_refuses_before_the_gpu(what):
    ctx = _NoGpu()                                           # 64 x 48; any native call would be an AttributeError
    good = _rle(2)
    kw = {}
    arg = {"wrong size": lambda: _rle(2, H=48, W=63),
           "33 masks": lambda: [good, _rle(33)],
           "start < 0": lambda: _spoiled("runs", np.array([[-1, 4]], np.int32)),
           "length < 0": lambda: _spoiled("runs", np.array([[3, -4]], np.int32)),
           "past the image": lambda: _spoiled("runs", np.array([[64 * 48 - 2, 3]], np.int32)),
           "float runs": lambda: _spoiled("runs", good.runs.astype(np.float32)),
           "flat runs": lambda: _spoiled("runs", good.runs.reshape(-1)),
           "offsets": lambda: _spoiled("run_off", good.run_off[::-1].copy()),
           "dense": lambda: [good, good.to_dense()],
           "erode_iters": lambda: good}[what]()
    if what in ("start < 0", "length < 0", "past the image"):
        arg.run_off = np.array([0, 1, 1], np.int64)
    if what == "erode_iters":
        kw = dict(erode_iters=-1)
    with pytest.raises(ValueError):
        ctx.set_masks_rle(arg, **kw)


class _Cam:
    width, height = 64, 48
    K = np.eye(3)


@pytest.mark.parametrize("what", ["mixed", "mixed, dense first", "wrong size"])
def test_run_frames_refuses_before_the_gpu(what):
    pts = np.zeros((10, 4), np.float32)
    dense = np.zeros((2, 48, 64), np.uint8)
    frames = {"mixed": [pipeline.FrameInputs(1, pts, _rle(2)), pipeline.FrameInputs(2, pts, dense)],
              "mixed, dense first": [pipeline.FrameInputs(1, pts, dense), pipeline.FrameInputs(2, pts, None), pipeline.FrameInputs(3, pts, _rle(2))],
              "wrong size": [pipeline.FrameInputs(1, pts, _rle(2, H=24, W=32))]}[what]
    with pytest.raises(ValueError):
        pipeline.run_frames(frames, np.eye(4), _Cam(), ctx=_NoGpu())
