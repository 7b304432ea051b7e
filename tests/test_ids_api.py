"""Instance-ID maps (lpf_set_masks_ids, lpf_run_wide_ids, idmap.IdMasks) without a GPU: the header declares the struct, the two calls
and LPF_ID_NONE under ABI 8, the ctypes mirror matches the C layout (compiled and measured by gcc) while the structs beside it keep
theirs, the library exports both entry points and carries every instantiation of the two decode kernels, IdMasks agrees with
``ids == sel[m]`` in NumPy, and the Python entries refuse bad input before anything reaches the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from lidar_object_detection_amd import _build, _native, pipeline
from lidar_object_detection_amd._native import IdMasksInput, RleMasksInput, WideInput, WideOutputs
from lidar_object_detection_amd.idmap import LPF_ID_NONE, IdMasks
from lidar_object_detection_amd.rle import RleMasks
from test_wide_api import HEADER, _NoGpu, _c_layout, _header_text


def test_header_declares_the_struct_the_calls_and_the_constant():
    text = re.sub(r"/\*.*?\*/", "", _header_text(), flags=re.S)
    assert re.search(r"\bint\s+lpf_set_masks_ids\s*\(\s*lpf_ctx\s*\*\s*\w*\s*,\s*const\s+lpf_id_masks\s*\*\s*\w*\s*\)", text)
    assert re.search(r"\bint\s+lpf_run_wide_ids\s*\(\s*lpf_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*\w*\s*,\s*const\s+int64_t\s*\*\s*\w*\s*,\s*int\s+\w*\s*,"
                     r"\s*int\s+\w*\s*,\s*const\s+lpf_id_masks\s*\*\s*\w*\s*,\s*const\s+lpf_wide_outputs\s*\*\s*\w*\s*\)", text)
    assert re.search(r"typedef\s+struct\s+lpf_id_masks\s*\{", text) and re.search(r"\}\s*lpf_id_masks\s*;", text)
    assert re.search(r"#define\s+LPF_ID_NONE\s+INT32_MIN\b", text)
    assert re.search(r"#define\s+LPF_ABI_VERSION\s+8\b", _header_text())
    assert "8 (continued): LPF_ID_NONE, lpf_id_masks, lpf_set_masks_ids, lpf_run_wide_ids (added; nothing else" in _header_text()
    assert "lpf_set_masks_ids" in _native.EXPORTED and "lpf_run_wide_ids" in _native.EXPORTED
    assert "lpf_ids.hip.h" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "lpf_ids.hip.h"))
    assert LPF_ID_NONE == -2 ** 31 and os.path.isfile(HEADER)


def test_struct_mirror_matches_the_header(tmp_path):
    names = [f[0] for f in IdMasksInput._fields_]
    assert names == ["ids", "sel", "F", "M", "id_bytes", "erode_iters", "on_device", "reserved"]
    lay = _c_layout(tmp_path, "lpf_id_masks", names)
    assert lay["sizeof"] == ctypes.sizeof(IdMasksInput) == 40
    for n in names:
        assert lay[n] == getattr(IdMasksInput, n).offset, n


@pytest.mark.parametrize("cls,struct,size", [(WideInput, "lpf_wide_input", 40), (RleMasksInput, "lpf_rle_masks", 32),
                                             (WideOutputs, "lpf_wide_outputs", 152)])
def test_the_structs_beside_it_keep_their_layout(cls, struct, size, tmp_path):
    names = [f[0] for f in cls._fields_]
    lay = _c_layout(tmp_path, struct, names)
    assert lay["sizeof"] == ctypes.sizeof(cls) == size
    for n in names:
        assert lay[n] == getattr(cls, n).offset, n


def test_the_constant_is_what_the_header_says(tmp_path):
    src = tmp_path / "none.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(void) { printf("%%d %%d\\n", (int)LPF_ID_NONE, LPF_ABI_VERSION); return 0; }\n' % HEADER)
    subprocess.check_call(["gcc", "-std=c99", str(src), "-o", str(tmp_path / "none")])
    out = subprocess.run([str(tmp_path / "none")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [LPF_ID_NONE, 8]


@pytest.mark.skipif(not os.path.exists(_build.LIB), reason="liblpf.so has not been built")
def test_library_carries_the_entry_points_and_the_decode_kernels():
    dyn = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT lpf_set_masks_ids\b", dyn) and re.search(r"\bT lpf_run_wide_ids\b", dyn)
    # (the host stubs: uint16 / int32 IDs x uint8 / uint16 / uint32 label elements, and the wide decode for both ID types)
    syms = subprocess.run(["nm", _build.LIB], check=True, capture_output=True, text=True).stdout
    for it in "ti":
        for lt in "htj":
            assert re.search(r"lpf_ids_labelI%s%sE" % (it, lt), syms), (it, lt)
        assert re.search(r"lpf_ids_planesI%sE" % it, syms), it


# ---- IdMasks ------------------------------------------------------------------------------------------------------------------------

def _map(H=48, W=64, dt=np.uint16, seed=0, n=20):
    return np.random.default_rng(seed).integers(0, n, (H, W)).astype(dt)


def _im(M, H=48, W=64, dt=np.uint16, seed=0):
    return IdMasks(_map(H, W, dt, seed), np.arange(M))


@pytest.mark.parametrize("dt", [np.uint16, np.int32])
def test_to_dense_is_ids_equal_sel(dt):
    ids = _map(23, 37, dt)
    if dt == np.int32:
        ids[3, 4:9] = LPF_ID_NONE
        ids[5, 5] = -1
    else:
        ids[5, 5] = 65535
    sel = [3, 7, 7, 100, -1, 65535, 65536 + 3, LPF_ID_NONE, 0]
    im = IdMasks(ids, sel)
    assert im.shape == (9, 23, 37) and len(im) == 9 and im.sel.dtype == np.int32 and im.ids is ids
    d = im.to_dense()
    assert d.dtype == np.uint8 and d.shape == (9, 23, 37)
    for m, v in enumerate(sel):
        want = np.zeros((23, 37), bool) if v == LPF_ID_NONE else ids.astype(np.int64) == v
        assert np.array_equal(d[m], want.astype(np.uint8)), m
    assert d[1].any() and np.array_equal(d[1], d[2]) and not d[3].any() and not d[6].any() and not d[7].any()
    assert d[4].sum() == (1 if dt == np.int32 else 0) and d[5].sum() == (0 if dt == np.int32 else 1)
    assert "IdMasks(M=9, H=23, W=37" in repr(im) and np.dtype(dt).name in repr(im)


def test_slices_share_the_map():
    im = _im(7)
    d = im.to_dense()
    for a, b in [(0, 7), (2, 5), (3, 4), (5, 5), (6, 100), (-2, None), (None, 3)]:
        s = im[a:b]
        assert isinstance(s, IdMasks) and s.ids is im.ids and s.shape == d[a:b].shape and len(s) == len(d[a:b])
        assert np.array_equal(s.to_dense(), d[a:b]), (a, b)
    with pytest.raises(TypeError):
        im[2]
    with pytest.raises(TypeError):
        im[::2]


def test_an_id_map_never_becomes_an_object_array():
    im = _im(2)
    with pytest.raises(TypeError, match="to_dense"):
        np.asarray(im)
    with pytest.raises(TypeError, match="to_dense"):
        np.array(im)


@pytest.mark.parametrize("dt", [np.int16, np.uint8, np.int64, np.uint32, np.float32, bool])
def test_other_dtypes_are_a_type_error_that_names_astype(dt):
    with pytest.raises(TypeError, match=r"\.astype"):
        IdMasks(np.zeros((4, 5), dt), [1])
    with pytest.raises(TypeError, match=r"\.astype"):
        IdMasks.from_instance_map(np.zeros((4, 5), dt))


def test_constructor_checks_shape_and_sel():
    ids = np.zeros((4, 5), np.uint16)
    assert IdMasks(ids, []).shape == (0, 4, 5)
    assert IdMasks(ids, [2 ** 31 - 1, -2 ** 31]).sel.tolist() == [2 ** 31 - 1, -2 ** 31]
    for bad in ([2 ** 31], [-2 ** 31 - 1], [1.5], [[1, 2]], ["a"]):
        with pytest.raises(ValueError):
            IdMasks(ids, bad)
    for shape in ((4,), (2, 4, 5), (0, 5)):
        with pytest.raises(ValueError):
            IdMasks(np.zeros(shape, np.uint16), [1])


def test_from_instance_map_on_a_hand_made_map():
    ids = np.array([[26001, 26001, 26002, 0], [26000, 11005, 26002, 26001], [0, 0, 11005, 26000]], np.uint16)
    im = IdMasks.from_instance_map(ids)
    assert im.sel.tolist() == [26001, 26002] and im.ids is ids         # ascending; 26000 (no instance), 11005 (another class) and 0 are left out
    assert np.array_equal(im.to_dense(), np.stack([ids == 26001, ids == 26002]).astype(np.uint8))
    assert IdMasks.from_instance_map(ids, class_id=11).sel.tolist() == [11005]
    assert IdMasks.from_instance_map(ids, class_id=26, divisor=100).sel.tolist() == []
    assert IdMasks.from_instance_map(ids.astype(np.int32), class_id=260, divisor=100).sel.tolist() == [26001, 26002]
    assert len(IdMasks.from_instance_map(np.zeros((3, 4), np.int32))) == 0


def test_ids_batch_pads_ragged_frames_and_stacks_host_maps():
    a, b, c = _im(3, seed=1), _im(0, seed=2), _im(5, seed=3)
    maps, sel, F, M, id_bytes, dev = _native.ids_batch([a, b, c], 48, 64)
    assert (F, M, id_bytes, dev) == (3, 5, 2, False) and maps.shape == (3, 48, 64) and maps.dtype == np.uint16 and maps.flags.c_contiguous
    assert np.array_equal(maps[0], a.ids) and np.array_equal(maps[2], c.ids)
    assert sel.dtype == np.int32 and sel.tolist() == [[0, 1, 2, LPF_ID_NONE, LPF_ID_NONE], [LPF_ID_NONE] * 5, [0, 1, 2, 3, 4]]
    one = _native.ids_batch(_im(3, dt=np.int32), 48, 64)
    assert one[2:] == (1, 3, 4, False) and one[0].shape == (1, 48, 64) and one[0].dtype == np.int32
    inp = _native._ids_input(maps, sel, F, M, id_bytes, dev, 2)
    assert (inp.ids, inp.sel, inp.F, inp.M, inp.id_bytes, inp.erode_iters, inp.on_device, inp.reserved) == \
        (maps.ctypes.data, sel.ctypes.data, 3, 5, 2, 2, 0, 0)


# ---- refusals before anything reaches the library -----------------------------------------------------------------------------------

def _spoiled_sel(value):
    im = _im(2)
    im.sel = value
    return im


REFUSALS = {"mixed with dense": lambda: [_im(2), _im(2).to_dense()],
            "mixed with rle": lambda: [_im(2), RleMasks.from_dense(_im(2).to_dense())],
            "wrong size": lambda: _im(2, H=48, W=63),
            "differing dtypes": lambda: [_im(2), _im(2, dt=np.int32)],
            "too many masks": lambda: [_im(2), _im(300)],
            "sel outside int32": lambda: _spoiled_sel(np.array([2 ** 31], np.int64)),
            "sel not flat": lambda: _spoiled_sel(np.zeros((2, 2), np.int32))}


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["33 masks", "erode_iters", "not id maps"])
def test_set_masks_ids_refuses_before_the_gpu(what):
    ctx = _NoGpu()                                           # 64 x 48; any native call would be an AttributeError
    kw = dict(erode_iters=-1) if what == "erode_iters" else {}
    arg = _im(33) if what == "33 masks" else _im(2) if what == "erode_iters" else _im(2).to_dense() if what == "not id maps" else REFUSALS[what]()
    with pytest.raises(ValueError):
        ctx.set_masks_ids(arg, **kw)


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["rects", "binarize", "erode_iters", "frame count", "257 masks"])
def test_run_wide_refuses_before_the_gpu(what):
    ctx = _NoGpu()
    pts = [np.zeros((10, 4), np.float32)]
    kw, arg = {}, _im(40)
    if what in REFUSALS:
        arg = REFUSALS[what]()
        pts = pts * (len(arg) if isinstance(arg, list) else 1)
    elif what == "rects":
        kw = dict(rects=np.zeros((40, 4), np.int32))
    elif what == "binarize":
        kw = dict(binarize="gt0.5")
    elif what == "erode_iters":
        kw = dict(erode_iters=-1)
    elif what == "frame count":
        arg = [_im(40), _im(40)]
    elif what == "257 masks":
        arg = _im(257)
    with pytest.raises(ValueError):
        ctx.run_wide(pts, arg, **kw)


class _Cam:
    width, height = 64, 48
    K = np.eye(3)


@pytest.mark.parametrize("what", ["mixed", "mixed, dense first", "mixed with rle", "wrong size", "differing dtypes"])
def test_run_frames_refuses_before_the_gpu(what):
    pts = np.zeros((10, 4), np.float32)
    dense = np.zeros((2, 48, 64), np.uint8)
    frames = {"mixed": [pipeline.FrameInputs(1, pts, _im(2)), pipeline.FrameInputs(2, pts, dense)],
              "mixed, dense first": [pipeline.FrameInputs(1, pts, dense), pipeline.FrameInputs(2, pts, None), pipeline.FrameInputs(3, pts, _im(2))],
              "mixed with rle": [pipeline.FrameInputs(1, pts, _im(2)), pipeline.FrameInputs(2, pts, RleMasks.from_dense(dense))],
              "wrong size": [pipeline.FrameInputs(1, pts, _im(2, H=24, W=32))],
              "differing dtypes": [pipeline.FrameInputs(1, pts, _im(2)), pipeline.FrameInputs(2, pts, _im(2, dt=np.int32))]}[what]

    class Ctx(_NoGpu):                                       # (run_frames sets the element and the camera first: host state here)
        def set_erosion_element(self, k):
            pass

        def set_camera(self, *a):
            pass

    with pytest.raises(ValueError):
        pipeline.run_frames(frames, np.eye(4), _Cam(), ctx=Ctx())
