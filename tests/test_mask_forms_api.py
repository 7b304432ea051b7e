"""The forms of masks (dense, run-length, instance-ID maps) through the one table of compact forms, without a GPU: every refusal the
entry points make for a compact form -- exception type and full text, recorded from the code before the forms shared one route -- and
which forms each entry point recognises: a form it does not take goes the dense way, to that path's own TypeError."""
import ctypes

import numpy as np
import pytest

from lidar_object_detection_amd import _native, pipeline
from lidar_object_detection_amd.idmap import LPF_ID_NONE, IdMasks
from lidar_object_detection_amd.rle import RleMasks
from test_wide_api import _NoGpu

H, W = 48, 64
PTS = [np.zeros((10, 4), np.float32)]
DENSE = np.zeros((2, H, W), np.uint8)


class FakeGpuMap:                                           # what _is_torch looks at: a type from a torch module, on the GPU
    is_cuda = True
    shape, dtype = (H, W), "torch.uint16"

    def __init__(self, ptr=0x1000):
        self._ptr = ptr

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr


FakeGpuMap.__module__ = "torch"


def _rle(M, H=H, W=W, seed=0):
    return RleMasks.from_dense((np.random.default_rng(seed).random((M, H, W)) < 0.1).astype(np.uint8))


def _im(M, H=H, W=W, dt=np.uint16, seed=0):
    return IdMasks(np.random.default_rng(seed).integers(0, 20, (H, W)).astype(dt), np.arange(M))


def _gpu_im(M, ptr=0x1000):
    return IdMasks(FakeGpuMap(ptr), np.arange(M))


MAKE = {"rle": _rle, "ids": _im}


def _cam(masks, **kw):
    return dict(T_velo_to_rect=np.eye(4), K=np.eye(3), width=W, height=H, masks=masks, **kw)


class _Cam:
    width, height = W, H
    K = np.eye(3)


class _Ctx(_NoGpu):                                          # (the pipeline sets the element and the camera first: host state here)
    def set_erosion_element(self, k):
        pass

    def set_camera(self, *a):
        pass


# ---- the entry points: any native call would be an AttributeError (no library is loaded) ---------------------------------------------
def run_wide(masks, F=1, **kw):
    return _NoGpu().run_wide(PTS * F, masks, **kw)


def depth_maps(masks, F=1, **kw):
    return _NoGpu().depth_maps(PTS * F, masks, **kw)


def run_cams(masks, F=1, **kw):                              # the masks are camera 1's: the prefix says so
    return _NoGpu().run_cams(PTS * F, [_cam(None), _cam(masks, **kw)])


def first_match(masks, F=1, colors=None):
    return _native.LpfContext.first_match_rle_batch(masks, colors, F)


def set_masks_ids(masks, **kw):
    return _NoGpu().set_masks_ids(masks, **kw)


def _frames(*masks):
    return [pipeline.FrameInputs(i + 1, PTS[0], m, colors=[(1, 2, 3)] * (len(m) if m is not None else 0)) for i, m in enumerate(masks)]


def run_frames(*masks):
    return pipeline.run_frames(_frames(*masks), np.eye(4), _Cam(), ctx=_Ctx())


def run_frames_multicam(*masks):                             # the masks are camera 1's frames
    cam0 = _frames(*[_rle(2) for _ in masks])
    return pipeline.run_frames_multicam([cam0, _frames(*masks)], [(np.eye(4), _Cam()), (np.eye(4), _Cam())], ctx=_Ctx())


def depth_maps_frames(*masks):
    return pipeline.depth_maps_frames(_frames(*masks), np.eye(4), _Cam(), ctx=_Ctx())


def first_match_frames(*masks):
    return pipeline.first_match_frames(_frames(*masks), np.eye(4), _Cam(), ctx=_Ctx())


# ---- the passes behind compact_mask_batch ------------------------------------------------------------------------------------------
# {who} is the entry point's prefix; {limit} / {over} the masks one pass takes and one more; {other} a binarize that is not its default
PASS_TEXTS = {
    "rle": {"mixed list": "{who}: the list mixes RleMasks and arrays: one form per call (.to_dense() or RleMasks.from_dense)",
            "mixed list, array first": "{who}: the list mixes RleMasks and arrays: one form per call (.to_dense() or RleMasks.from_dense)",
            "rects": "{who}: rects given with RleMasks (the runs say where the masks are)",
            "binarize": "{who}: binarize='{other}' with RleMasks (a pixel is a member or it is not)",
            "erode_iters negative": "erode_iters must be a non-negative integer, got -1",
            "erode_iters 1.5": "erode_iters must be a non-negative integer, got 1.5",
            "frame count": "{who}: RleMasks for 3 frames, the batch has 2",
            "wrong size": "{who}: frame 1 has masks of 63 x 48, the camera is 64 x 48 (runs are not resized)",
            "too many masks": "{who}: frame 1 has {over} masks, one pass takes {limit} (pipeline.run_frames groups them)"},
    "ids": {"mixed list": "{who}: the list mixes IdMasks with another form of masks: one form per call (.to_dense())",
            "mixed list, array first": "{who}: the list mixes IdMasks with another form of masks: one form per call (.to_dense())",
            "rects": "{who}: rects given with IdMasks (the map says where the masks are)",
            "binarize": "{who}: binarize='{other}' with IdMasks (a pixel is a member or it is not)",
            "erode_iters negative": "erode_iters must be a non-negative integer, got -1",
            "erode_iters 1.5": "erode_iters must be a non-negative integer, got 1.5",
            "frame count": "{who}: IdMasks for 3 frames, the batch has 2",
            "wrong size": "{who}: frame 1 has a map of 63 x 48, the camera is 64 x 48 (maps are not resized)",
            "too many masks": "{who}: frame 1 has {over} masks, one pass takes {limit} (pipeline.run_frames groups them)",
            "differing dtypes": "{who}: the frames' maps have differing ID dtypes ['int32', 'uint16']: one dtype per call",
            "host and GPU maps": "{who}: host and GPU maps in one call: one place per call",
            "GPU maps apart": "{who}: GPU maps must be the frames of ONE contiguous [F,H,W] tensor (IdMasks(t[f], sel)), or F = 1: frame 1 "
                              "is not where frame 0 + 1 frames is"}}
# (entry point, the message's prefix, its default binarize and another, masks per pass, the compact forms it takes)
PASSES = {"run_wide": (run_wide, "run_wide", "astype", "gt0.5", 256, ("rle", "ids")),
          "depth_maps": (depth_maps, "depth_maps", "gt0.5", "astype", 256, ("rle",)),
          "run_cams": (run_cams, "run_cams: camera 1", "astype", "gt0.5", 32, ("rle",))}


def _pass_call(call, form, what, other, limit):
    mk = MAKE[form]
    return {"mixed list": lambda: call([mk(2), DENSE], F=2),
            "mixed list, array first": lambda: call([DENSE, mk(2)], F=2),
            "rects": lambda: call(mk(2), rects=np.zeros((1, 2, 4), np.int32)),
            "binarize": lambda: call(mk(2), binarize=other),
            "erode_iters negative": lambda: call(mk(2), erode_iters=-1),
            "erode_iters 1.5": lambda: call(mk(2), erode_iters=1.5),
            "frame count": lambda: call([mk(2), mk(0), mk(3)], F=2),
            "wrong size": lambda: call([mk(2), mk(2, W=63)], F=2),
            "too many masks": lambda: call([mk(0), mk(limit + 1)], F=2),
            "differing dtypes": lambda: call([_im(2), _im(3, dt=np.int32)], F=2),
            "host and GPU maps": lambda: call([_gpu_im(2), _im(3)], F=2),
            "GPU maps apart": lambda: call([_gpu_im(2), _gpu_im(3, ptr=0x1000)], F=2)}[what]


@pytest.mark.parametrize("entry,form,what", [(e, f, w) for e in PASSES for f in PASSES[e][5] for w in PASS_TEXTS[f]])
def test_a_pass_refuses_a_compact_form_as_before(entry, form, what):
    call, who, _, other, limit, _ = PASSES[entry]
    with pytest.raises(ValueError) as e:
        _pass_call(call, form, what, other, limit)()
    assert str(e.value) == PASS_TEXTS[form][what].format(who=who, other=other, limit=limit, over=limit + 1)


# ---- everything else: (call, exception, full text) -----------------------------------------------------------------------------------
NOT_AN_ARRAY = "IdMasks is not an array: use .to_dense() for entry points that take dense masks"
NOT_AN_INDEX = "IdMasks takes slices over masks (im[a:b]), got 0"
MIXES_IDS = "the list mixes IdMasks with another form of masks: one form per call (.to_dense())"
RLE_BATCH_MIXED = "dense masks in a batch of RleMasks frames: one form per batch (.to_dense() or RleMasks.from_dense)"
IDS_BATCH_MIXED = "another form of masks in a batch of IdMasks frames: one form per batch (.to_dense())"
RLE_BATCH_SIZE = "RleMasks of 32 x 24, the camera is 64 x 48 (runs are not resized: decode with .to_dense())"
REFUSALS = {
    # a list that mixes the two compact forms: run_wide looks for ID maps first, run_frames for run-length masks
    "run_wide/both forms, rle first": (lambda: run_wide([_rle(2), _im(2)], F=2), ValueError, "run_wide: " + MIXES_IDS),
    "run_wide/both forms, ids first": (lambda: run_wide([_im(2), _rle(2)], F=2), ValueError, "run_wide: " + MIXES_IDS),
    "run_frames/both forms, rle first": (lambda: run_frames(_rle(2), _im(2)), ValueError, "frame 2: " + RLE_BATCH_MIXED),
    "run_frames/both forms, ids first": (lambda: run_frames(_im(2), _rle(2)), ValueError, "frame 1: " + RLE_BATCH_MIXED),
    # a form an entry point does not take is not recognised there: the dense path's TypeError
    "depth_maps/ids": (lambda: depth_maps(_im(2)), TypeError, NOT_AN_ARRAY),
    "depth_maps/ids, list": (lambda: depth_maps([_im(2), _im(3)], F=2), TypeError, NOT_AN_ARRAY),
    "run_cams/ids": (lambda: run_cams(_im(2)), TypeError, NOT_AN_ARRAY),
    "run_frames_multicam/ids": (lambda: run_frames_multicam(_im(2), _im(3)), TypeError, NOT_AN_ARRAY),
    "depth_maps_frames/ids": (lambda: depth_maps_frames(_im(2), _im(3)), TypeError, NOT_AN_INDEX),
    "first_match_frames/ids": (lambda: first_match_frames(_im(2), _im(3)), TypeError, NOT_AN_INDEX),
    "first_match/mixed list": (lambda: first_match([_rle(2), DENSE], F=2), ValueError,
                               "first_match: the list mixes RleMasks and arrays: one form per call (.to_dense() or RleMasks.from_dense)"),
    "first_match/frame count": (lambda: first_match([_rle(2), _rle(0), _rle(3)], F=2), ValueError,
                                "first_match: RleMasks for 3 frames, the batch has 2"),
    "first_match/differing sizes": (lambda: first_match([_rle(2), _rle(2, H=24, W=32)], F=2), ValueError,
                                    "first_match: the frames' RleMasks have differing sizes (H, W) = [(24, 32), (48, 64)]: one size per call "
                                    "(runs are not resized)"),
    "first_match/too many masks": (lambda: first_match(_rle(257)), ValueError,
                                   "first_match: frame 0 has 257 masks, one pass takes 256 (pipeline.run_frames groups them)"),
    "first_match/colors": (lambda: first_match(_rle(3), colors=np.zeros((1, 2, 3))), ValueError,
                           "first_match: colors [F,M,3] = (1, 3, 3), got (1, 2, 3)"),
    "set_masks_ids/dense": (lambda: set_masks_ids(DENSE), ValueError,
                            "set_masks_ids: masks must be an IdMasks or a list of them, got ndarray"),
    "set_masks_ids/rle": (lambda: set_masks_ids(_rle(2)), ValueError,
                          "set_masks_ids: masks must be an IdMasks or a list of them, got RleMasks"),
    "set_masks_ids/list of rle": (lambda: set_masks_ids([_rle(2)]), ValueError,
                                  "set_masks_ids: masks must be an IdMasks or a list of them, got list"),
    "set_masks_ids/mixed list": (lambda: set_masks_ids([_im(2), DENSE]), ValueError, "set_masks_ids: " + MIXES_IDS),
    "set_masks_ids/erode_iters negative": (lambda: set_masks_ids(_im(2), erode_iters=-1), ValueError,
                                           "erode_iters must be a non-negative integer, got -1"),
    "set_masks_ids/erode_iters 1.5": (lambda: set_masks_ids(_im(2), erode_iters=1.5), ValueError,
                                      "erode_iters must be a non-negative integer, got 1.5"),
    "set_masks_ids/wrong size": (lambda: set_masks_ids([_im(2), _im(2, W=63)]), ValueError,
                                 "set_masks_ids: frame 1 has a map of 63 x 48, the camera is 64 x 48 (maps are not resized)"),
    "set_masks_ids/too many masks": (lambda: set_masks_ids([_im(0), _im(33)]), ValueError,
                                     "set_masks_ids: frame 1 has 33 masks, one pass takes 32 (pipeline.run_frames groups them)"),
    "set_masks_ids/differing dtypes": (lambda: set_masks_ids([_im(2), _im(3, dt=np.int32)]), ValueError,
                                       "set_masks_ids: the frames' maps have differing ID dtypes ['int32', 'uint16']: one dtype per call"),
    "set_masks_ids/host and GPU maps": (lambda: set_masks_ids([_gpu_im(2), _im(3)]), ValueError,
                                        "set_masks_ids: host and GPU maps in one call: one place per call"),
    # set_masks_rle keeps its own erosion check, with its own words
    "set_masks_rle/erode_iters negative": (lambda: _NoGpu().set_masks_rle(_rle(2), erode_iters=-1), ValueError,
                                           "erode_iters must be >= 0, got -1"),
    "set_masks_rle/ids": (lambda: _NoGpu().set_masks_rle([_im(2)]), ValueError, "set_masks_rle: frame 0 is IdMasks, not RleMasks"),
    "run_frames/rle/mixed": (lambda: run_frames(_rle(2), DENSE), ValueError, "frame 2: " + RLE_BATCH_MIXED),
    "run_frames/rle/mixed, dense first": (lambda: run_frames(DENSE, None, _rle(2)), ValueError, "frame 1: " + RLE_BATCH_MIXED),
    "run_frames/rle/wrong size": (lambda: run_frames(_rle(0), _rle(2, H=24, W=32)), ValueError, "frame 2: " + RLE_BATCH_SIZE),
    "run_frames/ids/mixed": (lambda: run_frames(_im(2), DENSE), ValueError, "frame 2: " + IDS_BATCH_MIXED),
    "run_frames/ids/mixed, dense first": (lambda: run_frames(DENSE, None, _im(2)), ValueError, "frame 1: " + IDS_BATCH_MIXED),
    "run_frames/ids/wrong size": (lambda: run_frames(_im(0), _im(2, H=24, W=32)), ValueError,
                                  "frame 2: an ID map of 32 x 24, the camera is 64 x 48 (maps are not resized: use .to_dense())"),
    "run_frames/ids/differing dtypes": (lambda: run_frames(_im(2), _im(3, dt=np.int32)), ValueError,
                                        "set_masks_ids: the frames' maps have differing ID dtypes ['int32', 'uint16']: one dtype per call"),
    "run_frames/ids/no masks among GPU maps": (lambda: run_frames(_gpu_im(2), None), ValueError,
                                               "frame 2: no masks in a batch of GPU ID maps: give it IdMasks(t[f], []) over its frame of the "
                                               "batch's tensor"),
    "run_frames/ids/host and GPU maps": (lambda: run_frames(_gpu_im(2), _im(3)), ValueError,
                                         "set_masks_ids: host and GPU maps in one call: one place per call"),
    "run_frames_multicam/rle/mixed": (lambda: run_frames_multicam(_rle(2), DENSE), ValueError, "frame 2: " + RLE_BATCH_MIXED),
    "run_frames_multicam/rle/wrong size": (lambda: run_frames_multicam(_rle(2, H=24, W=32), None), ValueError, "frame 1: " + RLE_BATCH_SIZE),
    "depth_maps_frames/rle/mixed": (lambda: depth_maps_frames(_rle(2), DENSE), ValueError, "frame 2: " + RLE_BATCH_MIXED),
    "depth_maps_frames/rle/wrong size": (lambda: depth_maps_frames(_rle(2), _rle(2, H=24, W=32)), ValueError, "frame 2: " + RLE_BATCH_SIZE),
    "first_match_frames/rle/mixed": (lambda: first_match_frames(_rle(2), DENSE), ValueError, "frame 2: " + RLE_BATCH_MIXED),
    "first_match_frames/rle/differing sizes": (lambda: first_match_frames(_rle(2), _rle(2, H=24, W=32)), ValueError,
                                               "first_match_frames: the frames' RleMasks have differing sizes (H, W) = [(24, 32), (48, 64)]: "
                                               "one size per batch (runs are not resized: decode with .to_dense())"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_a_refusal_keeps_its_type_and_text(what):
    call, exc, text = REFUSALS[what]
    with pytest.raises(exc) as e:
        call()
    assert type(e.value) is exc and str(e.value) == text


# ---- which forms are recognised where ----------------------------------------------------------------------------------------------
def test_the_table_has_the_two_forms():
    assert [(f.name, f.cls) for f in _native.MASK_FORMS] == [("rle", RleMasks), ("ids", IdMasks)]


@pytest.mark.parametrize("masks", [DENSE, [DENSE], None, [], "rle", 3])
def test_the_recogniser_leaves_other_arguments_alone(masks):
    assert _native.compact_frames(masks, "who", ("rle", "ids")) is None
    assert _native.compact_mask_batch(masks, 1, H, W, forms=("rle", "ids")) is None


def test_the_recogniser_takes_only_the_forms_it_is_given():
    r, i = _rle(2), _im(2)
    for masks, form in ((r, "rle"), ([r, r], "rle"), ((r,), "rle"), (i, "ids"), ([i, i], "ids")):
        other = "ids" if form == "rle" else "rle"
        found, frames = _native.compact_frames(masks, "who", (form,))
        assert found.name == form and frames == (list(masks) if isinstance(masks, (list, tuple)) else [masks])
        assert _native.compact_frames(masks, "who", (other, form))[0].name == form
        assert _native.compact_frames(masks, "who", (other,)) is None
        assert _native.compact_frames(masks, "who", ()) is None
    # an ID map handed to depth_maps' resolver is "not compact"; the dense path then says what to do
    assert _native.compact_mask_batch(i, 1, H, W, binarize="gt0.5", who="depth_maps", default_binarize="gt0.5", forms=("rle",)) is None
    with pytest.raises(TypeError, match=r"\.to_dense\(\)"):
        np.asarray(i)
    assert _native.LpfContext.first_match_rle_batch(i, None, 1) is None and _native.LpfContext.first_match_rle_batch([i], None, 1) is None


@pytest.mark.parametrize("forms", [("rle",), ("ids",), ("rle", "ids"), ("ids", "rle")])
def test_the_collector_takes_only_the_forms_it_is_given(forms):
    for form, mk in MAKE.items():
        frames = _frames(mk(2), None, mk(3))
        found = pipeline._compact_frame_masks(frames, _Cam(), forms)
        if form not in forms:
            assert found is None
            continue
        assert found[0] == form and found[1][0] is frames[0].masks and found[1][2] is frames[2].masks
        assert type(found[1][1]) is type(frames[0].masks) and found[1][1].shape == (0, H, W)
    assert pipeline._compact_frame_masks(_frames(DENSE, None), _Cam(), forms) is None


# ---- what the one function builds: F = 3 with ragged M (0, 2, 3) ---------------------------------------------------------------------
def test_compact_mask_batch_names_what_it_built():
    rle = _native.compact_mask_batch([_rle(0), _rle(2, seed=1), _rle(3, seed=2)], 3, H, W, erode_iters=1, forms=("ids", "rle"))
    runs, off = rle.tables
    assert (rle.form, rle.M, rle.is_float, rle.on_device, rle.masks, rle.rects, rle.gpu) == ("rle", 3, False, False, None, None, None)
    assert isinstance(rle.struct, _native.RleMasksInput) and off.shape == (3 * 3 + 1,) and off[3] == 0 and off[-1] == len(runs)
    assert (rle.struct.runs, rle.struct.run_off, rle.struct.F, rle.struct.M, rle.struct.erode_iters) == \
        (runs.ctypes.data, off.ctypes.data, 3, 3, 1)
    ids = _native.compact_mask_batch([_im(0), _im(2, seed=1), _im(3, seed=2)], 3, H, W, erode_iters=1, forms=("ids", "rle"))
    maps, sel = ids.tables
    assert (ids.form, ids.M, ids.is_float, ids.on_device, ids.masks, ids.rects, ids.gpu) == ("ids", 3, False, False, None, None, None)
    assert isinstance(ids.struct, _native.IdMasksInput) and maps.shape == (3, H, W) and maps.dtype == np.uint16
    assert sel.tolist() == [[LPF_ID_NONE] * 3, [0, 1, LPF_ID_NONE], [0, 1, 2]]
    s = ids.struct
    assert (s.ids, s.sel, s.F, s.M, s.id_bytes, s.erode_iters, s.on_device) == (maps.ctypes.data, sel.ctypes.data, 3, 3, 2, 1, 0)
    gpu = _native.compact_mask_batch(_gpu_im(3), 1, H, W, forms=("ids",))
    assert gpu.on_device is True and gpu.gpu is gpu.tables[0][0] and gpu.struct.ids == 0x1000 and gpu.struct.on_device == 1


def test_the_call_of_a_batch():
    """_masks_call: a compact form with a native function of its own takes its struct; one without rides in the lpf_wide_input."""
    ctx = _NoGpu()
    natives = {"dense": "wide", "ids": "wide_ids"}
    ids = _native.compact_mask_batch(_im(3), 1, H, W, erode_iters=2, forms=("ids", "rle"))
    assert ctx._masks_call(ids, "astype", 2, natives) == ("wide_ids", ids.struct, ids)
    rle = _native.compact_mask_batch(_rle(3), 1, H, W, erode_iters=2, forms=("ids", "rle"))
    fn, inp, keep = ctx._masks_call(rle, "astype", 2, natives)
    assert fn == "wide" and keep is rle and isinstance(inp, _native.WideInput)
    assert (inp.masks, inp.rects, inp.M, inp.f32, inp.binarize, inp.erode_iters, inp.on_device) == \
        (ctypes.addressof(rle.struct), None, 3, _native.LPF_MASKS_RLE, 0, 2, 0)
    assert ctx._masks_call(rle, "gt0.5", 2, {"dense": "dm", "rle": "dm_rle"}) == ("dm_rle", rle.struct, rle)
    dense = _native.wide_mask_batch(np.ones((1, 3, H, W), np.float32), 1, H, W, erode_iters=2, binarize="gt0.5")
    fn, inp, keep = ctx._masks_call(dense, "gt0.5", 2, {"dense": "dm", "rle": "dm_rle"})
    assert fn == "dm" and keep is dense
    assert (inp.masks, inp.rects, inp.M, inp.f32, inp.binarize, inp.erode_iters, inp.on_device) == \
        (dense.masks.ctypes.data, None, 3, 1, 2, 2, 0)
